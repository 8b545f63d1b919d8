// lf_zk_i8.hip -- the z_k build (launch_recompose_crt in bit-plane mode, L = 4) on the int8 matrix cores (gfx950 v_mfma_i32_32x32x32_i8):
//     out_k[plane][off + i] = CRT( sum_l B^l digit_k(planes[c][4 i + l]) )[plane]             (digit_k(v) = sign(v) bit_k(|v|))
// was k_recompose_crt_b4: per thread and bit-plane a 12-product butterfly (crt8) and 8 twiddle products on the 64-bit multiplier, VALU-issue-bound at 2.6 x
// the time its stores need -- to transform a vector whose 32 inputs per residue class are ternary digits.
//
// For one residue class u of the coefficient index (c = u + 3 q, q < 8) the 8 output words are F_p-linear in the 32 digits d[q][l]:
//     word(u, p) = sum_{q,l} T_u[p][(q,l)] d[q][l],      T_u[p][(q,l)] = (CRT coefficient of the installed tables, twiddle included) * B^l mod p.
// T is data: zk_i8_prepare pushes the 96 unit inputs (coefficient c, value B^l) through the generic k_recompose_crt and cuts the answers.  Every entry is
// written with eight balanced base-256 digits (in [-128, 127], of the entry or of the entry - p, whichever they can express: their reach ends at 0x7F7F..7F);
// the GEMM of one class then has 64 rows (p, byte) = two 32-row tiles, an inner dimension of (q, l) = 32 exactly and 32 columns = 32 consecutive elements i
// of ONE bit-plane k.  A and B meet position by position inside a lane half, so the hardware's order of the inner positions does not matter.
//
// Row m = 8 j + 4 h + r of tile t is (p, byte) = (2 j + h, r + 4 t): register 4 j + r of lane (n, h) is that row in column n, so a lane ends up with all
// eight byte sums s_0 .. s_7 of the words p = h, 2 + h, 4 + h, 6 + h of ITS element and recombines them without an exchange:
//     |s_b| <= 32 * 128 = 4096; with biases beta_b >= 4096 whose sum beta_b 256^b is 17 p the sums s_b + beta_b are non-negative and the word unchanged mod p:
//     X = s_0 + 2^8 s_1 + 2^16 s_2,  Y = s_3 + 2^8 s_4 + 2^16 s_5 (both below 2^30: 32-bit shifts and adds),  Z = s_6 + 2^8 s_7 < 2^22 (biases included),
//     word + 17 p = X + 2^24 (Y + 2^24 Z) < 2^71: one fq_reduce128_loose, no 64-bit product anywhere.
// The results are canonical residues, as those of k_recompose_crt_b4 are: the two kernels agree word for word.
#include <hip/hip_runtime.h>

#include <vector>

#include "lf_common.h"
#include "lf_field.cuh"
#include "lf_kernels.h"
#include "lf_i8_mma.cuh"

namespace lf {
using namespace i8mma;
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr size_t ZK_A_WORDS = 3 * 2 * 64 * 4;   // the A operands [class][tile][lane] x 16 bytes, then the 24 output planes [class][p], then the three biases
constexpr size_t ZK_TAB_WORDS = ZK_A_WORDS + 24 + 3;

// the digits of bit kk of four plane entries (byte l of mag = eight magnitude bits of entry l; byte l of sgn = 0xFF for a negative entry, else 0x01)
typedef unsigned short zk_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int zk_digits(u32 mag, u32 sgn, u32 kk) {
    const u32 t = (mag >> kk) & 0x01010101u;
    // 0x01 -> 0xFF per byte as a packed 16-bit product (0x0101 * 0xFF = 0xFFFF: no overflow; full rate, where t * 255 in 32 bits is a quarter-rate product),
    // then +1 / -1 by the sign byte
    const zk_us2 m = __builtin_bit_cast(zk_us2, t) * zk_us2{255, 255};
    return (int)(__builtin_bit_cast(u32, m) & sgn);
}

// wave = 32 elements of one residue class (blockIdx.y); lane (n, h) = (lane & 31, lane >> 5) loads the entries q = 4 h .. 4 h + 3 of element n -- 16
// contiguous bytes each -- ONCE and cuts all K bit-planes from registers; it stores the words p = 2 j + h of that element (256 contiguous bytes per lane half)
// (waves_per_eu: with at most 128 registers per lane the MFMAs write VGPRs -- no accumulator-register reads in front of the recombination)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_recompose_crt_i8(const int *tab, const int32_t *planes, size_t n_planes, u32 wit_len, u32 K, u64 *out, size_t ldz, size_t off) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nn = lane & 31, h = lane >> 5, u = blockIdx.y;
    const size_t i0 = ((size_t)blockIdx.x * 4 + wave) * 32;
    if (i0 >= wit_len) return;                    // (the whole wave)
    const size_t i = i0 + nn;
    const bool live = i < wit_len;
    const size_t li = live ? i : 0;               // a lane past the end loads element 0 (its column is its own) and stores nothing
    const v4i a0 = *(const v4i *)(tab + ((u * 2 + 0) * 64 + lane) * 4), a1 = *(const v4i *)(tab + ((u * 2 + 1) * 64 + lane) * 4);
    size_t orow[4];
#pragma unroll
    for (int j = 0; j < 4; j++) orow[j] = (size_t)tab[ZK_A_WORDS + 8 * u + 2 * j + h] * ldz + off + i;
    const u32 bX = (u32)tab[ZK_A_WORDS + 24], bY = (u32)tab[ZK_A_WORDS + 25], bZ = (u32)tab[ZK_A_WORDS + 26];
    int4 w[4];
#pragma unroll
    for (int jj = 0; jj < 4; jj++) w[jj] = *(const int4 *)(planes + (size_t)(u + 3 * (4 * h + jj)) * n_planes + 4 * li);
    u32 sgn[4];
#pragma unroll
    for (int jj = 0; jj < 4; jj++)
        sgn[jj] = (w[jj].x < 0 ? 0xFFu : 1u) | (w[jj].y < 0 ? 0xFF00u : 0x100u) | (w[jj].z < 0 ? 0xFF0000u : 0x10000u) | (w[jj].w < 0 ? 0xFF000000u : 0x1000000u);
    for (u32 kb = 0; kb < K; kb += 8) {
        u32 mag[4];
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const u32 m0 = (u32)(w[jj].x < 0 ? -w[jj].x : w[jj].x), m1 = (u32)(w[jj].y < 0 ? -w[jj].y : w[jj].y), m2 = (u32)(w[jj].z < 0 ? -w[jj].z : w[jj].z),
                      m3 = (u32)(w[jj].w < 0 ? -w[jj].w : w[jj].w);
            mag[jj] = ((m0 >> kb) & 0xFFu) | (((m1 >> kb) & 0xFFu) << 8) | (((m2 >> kb) & 0xFFu) << 16) | (((m3 >> kb) & 0xFFu) << 24);
        }
#pragma unroll
        for (u32 kk = 0; kk < 8; kk++) {
            if (kb + kk >= K) break;
            const v4i b = v4i{zk_digits(mag[0], sgn[0], kk), zk_digits(mag[1], sgn[1], kk), zk_digits(mag[2], sgn[2], kk), zk_digits(mag[3], sgn[3], kk)};
            const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const v16i c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b, zero, 0, 0, 0), c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b, zero, 0, 0, 0);
            u64 *o = out + (size_t)(kb + kk) * 24 * ldz;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                // (the biases make every sum non-negative and add up to a multiple of p: X, Y < 2^30, Z < 2^22)
                const u32 X = (u32)(c0[4 * j] + 256 * c0[4 * j + 1] + 65536 * c0[4 * j + 2]) + bX;
                const u32 Y = (u32)(c0[4 * j + 3] + 256 * c1[4 * j] + 65536 * c1[4 * j + 1]) + bY;
                const u32 Z = (u32)(c1[4 * j + 2] + 256 * c1[4 * j + 3]) + bZ;
                const u64 T = (u64)Y + ((u64)Z << 24);                   // word + 17 p = X + 2^24 T < 2^71
                const u64 lo = (T << 24) + X;
                const u64 hi = (T >> 40) + (lo < X);
                if (live) o[orow[j]] = fq_canon(fq_reduce128_loose(lo, hi));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// The matrix of the installed tables for the base B, in operand order (set-up: the tables and B do not change from step to step).  Synchronises s.
// zk->state: 1 = ready, -1 = these tables are not of the form the kernel needs (the caller keeps k_recompose_crt_b4).  Returns 0, or -1 for a HIP error.
int zk_i8_prepare(const DevCrt &t, u64 B, ZkI8 *zk, hipStream_t s) {
    zk->state = 0;
    zk->B = B;
    // unit input e = 4 c + l: coefficient c of element e is the digit vector (l-th digit 1), i.e. the value B^l
    std::vector<int32_t> hp((size_t)24 * 384, 0);
    for (int c = 0; c < 24; c++)
        for (int l = 0; l < 4; l++) hp[(size_t)c * 384 + (size_t)(4 * c + l) * 4 + l] = 1;
    std::vector<u64> U((size_t)24 * 96);
    void *scratch = nullptr;
    const size_t pb = hp.size() * 4, ub = U.size() * 8;
    if (!zk->dev && lf_dev_malloc(&zk->dev, ZK_TAB_WORDS * 4) != hipSuccess) return -1;
    if (lf_dev_malloc(&scratch, pb + ub) != hipSuccess) return -1;
    int32_t *dp = (int32_t *)scratch;
    u64 *du = (u64 *)((char *)scratch + pb);
    bool ok = hipMemcpyAsync(dp, hp.data(), pb, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        launch_recompose_crt(t, dp, 384, 96, 4, B, 1, 0, du, 96, 0, s);   // mode 0: the generic kernel
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(U.data(), du, ub, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    (void)hipFree(scratch);
    if (!ok) return -1;
    // output plane w belongs to the class whose inputs reach it: exactly one class per plane, eight planes per class (ascending: p = 0 .. 7)
    std::vector<int> tab(ZK_TAB_WORDS, 0);
    int cnt[3] = {0, 0, 0}, pl[3][8];
    for (int w = 0; w < 24; w++) {
        int cls = -1;
        for (int e = 0; e < 96; e++) {
            U[(size_t)w * 96 + e] = fq_canon(U[(size_t)w * 96 + e]);
            if (U[(size_t)w * 96 + e] == 0) continue;
            const int ue = (e / 4) % 3;
            if (cls >= 0 && cls != ue) { zk->state = -1; return 0; }
            cls = ue;
        }
        if (cls < 0 || cnt[cls] == 8) { zk->state = -1; return 0; }
        pl[cls][cnt[cls]++] = w;
    }
    for (int u = 0; u < 3; u++)
        for (int p = 0; p < 8; p++) tab[ZK_A_WORDS + 8 * u + p] = pl[u][p];
    // lane (m, h) of tile tl: row m = 8 j + 4 h' + r is (p, byte) = (2 j + h', r + 4 tl); its register jj holds the inner positions q = 4 h + jj, byte l
    for (int u = 0; u < 3; u++)
        for (int p = 0; p < 8; p++)
            for (int q = 0; q < 8; q++)
                for (int l = 0; l < 4; l++) {
                    const u64 T = U[(size_t)pl[u][p] * 96 + 4 * (u + 3 * q) + l];
                    __int128 v = T > 0x7F7F7F7F7F7F7F7Full ? (__int128)T - (__int128)LF_P : (__int128)T;
                    for (int byte = 0; byte < 8; byte++) {
                        const int d = (int)(int8_t)(unsigned char)(v & 0xFF);
                        v = (v - d) / 256;
                        const int tl = byte >> 2, m = 8 * (p >> 1) + 4 * (p & 1) + (byte & 3), ln = 32 * (q >> 2) + m;
                        tab[((size_t)(u * 2 + tl) * 64 + ln) * 4 + (q & 3)] |= (int)(((u32)d & 0xFFu) << (8 * l));
                    }
                    if (v != 0) { zk->state = -1; return 0; }
                }
    // biases beta_b = 4096 + n_b >= max |s_b| with sum_b beta_b 256^b = 17 p: n = the base-256 digits of 17 p - 4096 (2^64 - 1) / 255 (the top one takes the rest)
    {
        __int128 N = (__int128)17 * (__int128)LF_P - (__int128)4096 * (__int128)0x0101010101010101ull;
        u32 beta[8];
        for (int b = 0; b < 8; b++) {
            const u32 nb = b < 7 ? (u32)(N & 0xFF) : (u32)N;
            beta[b] = 4096 + nb;
            N >>= 8;
        }
        if (beta[7] >= 4096 + 256) { zk->state = -1; return 0; }
        tab[ZK_A_WORDS + 24] = (int)(beta[0] + 256 * beta[1] + 65536 * beta[2]);
        tab[ZK_A_WORDS + 25] = (int)(beta[3] + 256 * beta[4] + 65536 * beta[5]);
        tab[ZK_A_WORDS + 26] = (int)(beta[6] + 256 * beta[7]);
    }
    if (hipMemcpyAsync(zk->dev, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return -1;
    zk->state = 1;
    return 0;
}

// Result: lf_i8_launch.h (shape not handled: the caller launches k_recompose_crt_b4)
int launch_recompose_crt_i8(const ZkI8 &zk, const int32_t *planes, size_t n_planes, u32 wit_len, u32 K, u64 *out, size_t ldz, size_t off, hipStream_t s) {
    if (zk.state != 1 || !zk.dev || wit_len == 0 || K < 1 || K > 32 || (n_planes & 3) || ((uintptr_t)planes & 15) || ((uintptr_t)out & 7)) return I8_ERR_SHAPE;
    hipLaunchKernelGGL(k_recompose_crt_i8, dim3((wit_len + 127) / 128, 3), dim3(256), 0, s, (const int *)zk.dev, planes, n_planes, wit_len, K, out, ldz, off);
    return i8_launched();
}
}  // namespace lf
