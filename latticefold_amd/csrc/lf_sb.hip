// lf_sb.hip -- kernels of the small-base path (b = 4, 8, 16; lf_sb.h): the part cut, the evaluations of the digit planes, their share of G, the folding
// sumcheck round at degree 2b (nifs/folding/utils.rs:273-325), the first table materialisation and the fold of the witnesses (folding.rs:258-268).
// Written for correctness and plain structure: one product, one reduction -- none of the look-up-table / int8 GEMM forms of the b = 2 rounds.
#include "lf_sb.h"

#include "lf_i8g_dec.cuh"
#include "lf_kernels_dev.cuh"

namespace lf {
namespace {
__device__ __forceinline__ int sb_digit(const unsigned char *p) { return (int)*p - 64; }
inline int sb_launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
}  // namespace

// ---- part cut: one thread per (coefficient c, tile of 8 columns): K operand words ---------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sb_cut(const int32_t *planes, size_t N, u32 K, u32 lb, int mode, unsigned long long *D, size_t ldw) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= ldw * 24) return;
    const size_t T = gid % ldw;
    const u32 c = (u32)(gid / ldw);
    lfdec::DigitChain ch[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const size_t j = T * 8 + q;
        const int32_t v = j < N ? planes[(size_t)c * N + j] : 0;
        ch[q].init(fq_from_i64(v), LF_P);
    }
    for (u32 k = 0; k < K; k++) {
        unsigned long long w = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) w |= (unsigned long long)((ch[q].next(lb, mode) + 64) & 127) << (8 * q);
        D[((size_t)k * 24 + c) * ldw + T] = w;
    }
}
int launch_sb_cut(const int32_t *planes, size_t N, u32 K, u32 lb, int mode, unsigned char *D, size_t ldn, hipStream_t s) {
    const size_t ldw = ldn / 8;
    if (!N || ldn < N || (ldn & 7) || lb < 2 || lb > 4) return -1;
    hipLaunchKernelGGL(k_sb_cut, dim3(cdiv(ldw * 24, 256)), dim3(256), 0, s, planes, N, K, lb, mode, (unsigned long long *)D, ldw);
    return sb_launched();
}

// ---- evaluations: out[k][c][q] = sum_i eq[q][i] * digit.  |digit| <= 8: signed 128-bit sums per thread (2^20 columns: < 2^88), one reduction per thread ----
constexpr u32 SB_EVAL_BLOCKS = 64;
size_t sb_eval_partial_words(u32 K) { return (size_t)SB_EVAL_BLOCKS * K * 72; }
__global__ void __launch_bounds__(256) k_sb_eval(const unsigned char *D, size_t ldn, size_t n, const u64 *eq, size_t ldeq, u32 K, u64 *partial) {
    const u32 c = blockIdx.y, k = blockIdx.z;
    const unsigned char *row = D + ((size_t)k * 24 + c) * ldn;
    __int128 acc[3] = {0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int d = sb_digit(row + i);
        if (d == 0) continue;
#pragma unroll
        for (int q = 0; q < 3; q++) acc[q] += (__int128)eq[(size_t)q * ldeq + i] * d;   // (eq < 2^64, |d| <= 8)
    }
    u64 v[3];
#pragma unroll
    for (int q = 0; q < 3; q++) v[q] = fq_from_s128((u64)acc[q], (int64_t)(acc[q] >> 64));
    __shared__ u64 red[3];
    block_sum_store<3>(v, red);
    __syncthreads();
    if (threadIdx.x < 3) partial[(size_t)blockIdx.x * K * 72 + ((size_t)k * 24 + c) * 3 + threadIdx.x] = red[threadIdx.x];
}
int launch_sb_eval(const unsigned char *D, size_t ldn, size_t n, const u64 *eq, size_t ldeq, u32 K, u64 *partial, u64 *out, hipStream_t s) {
    if (!n || !K) return -1;
    u32 gb = cdiv(n, 256);
    if (gb > SB_EVAL_BLOCKS) gb = SB_EVAL_BLOCKS;
    hipLaunchKernelGGL(k_sb_eval, dim3(gb, 24, K), dim3(256), 0, s, D, ldn, n, eq, ldeq, K, partial);
    if (sb_launched()) return -1;
    hipLaunchKernelGGL(k_reduce_rows, dim3(K * 72), dim3(256), 0, s, partial, gb, K * 72, out);
    return sb_launched();
}

// ---- G[row][slot] += sum_k sum_d apow[k][d] * digit(D[k][8d + slot][row]) ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sb_add_fhat_comb(const unsigned char *D, size_t ldn, size_t n, u32 K, const Fq3Const *apow, u64 *G, size_t m) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u32 slot = blockIdx.y;
    if (row >= n) return;
    Fq3 acc = ld3(G, m, slot, row);
    for (u32 k = 0; k < K; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const int dg = sb_digit(D + ((size_t)k * 24 + 8 * d + slot) * ldn + row);
            if (dg == 0) continue;
            const Fq3Const a = apow[k * 3 + d];
            const Fq3 term = fq3_mul_small(fq3_make(a.c[0], a.c[1], a.c[2]), dg < 0 ? -dg : dg);
            acc = dg < 0 ? fq3_sub(acc, term) : fq3_add(acc, term);
        }
    st3(G, m, slot, row, acc);
}
int launch_sb_add_fhat_comb(const unsigned char *D, size_t ldn, size_t n, u32 K, const Fq3Const *apow_dev, u64 *G, size_t m, hipStream_t s) {
    if (n > m) n = m;
    if (!n) return 0;
    hipLaunchKernelGGL(k_sb_add_fhat_comb, dim3(cdiv(n, 256), 8), dim3(256), 0, s, D, ldn, n, K, apow_dev, G, m);
    return sb_launched();
}

// ---- the round: norm part at degree 2b ----------------------------------------------------------------------------------------------------------------------
// Grid (blocks, 8 slots, chunks): a block evaluates XC = 9 consecutive points X of the 2b + 1 (one chunk for b = 4, two for b = 8, four for b = 16), so that the
// per-point sums stay in registers.  Per pair and table the entries f0, f1 are read once; f(X) = f0 + X (f1 - f0) steps by additions.
constexpr int SB_XC = 9;
constexpr u32 SB_MAX_CHUNKS = 4;
size_t sb_round_out_words() { return (size_t)SB_MAX_CHUNKS * SB_XC * 24; }
size_t sb_round_partial_words() { return (size_t)RED_BLOCKS * sb_round_out_words(); }
template <bool NU, int B, bool TAB>
__global__ void __launch_bounds__(256) k_sb_round(DevCrt t, FoldRoundArgs a, const u64 *F, size_t ldF, const unsigned char *DL, const unsigned char *DR, size_t ldn,
                                                  size_t n_planes, u32 K, const Fq3Const *mu_pow, u64 *partial, u32 nv) {
    const u32 slot = blockIdx.y, X0 = blockIdx.z * SB_XC;
    const size_t pend = a.p0 + a.pcnt;
    Fq3 acc[SB_XC];
#pragma unroll
    for (int i = 0; i < SB_XC; i++) acc[i] = fq3_zero();
    for (size_t p = a.p0 + (size_t)blockIdx.x * 256 + threadIdx.x; p < pend; p += (size_t)gridDim.x * 256) {
        Fq3 S[SB_XC];
#pragma unroll
        for (int i = 0; i < SB_XC; i++) S[i] = fq3_zero();
        if (TAB) {
            for (u32 tb = 0; tb < 2 * K * 3; tb++) {
                const u64 *fp = F + ((size_t)tb * 24 + 3 * slot) * ldF + 2 * (p - a.pF0);
                const ulonglong2 a0 = *(const ulonglong2 *)fp, a1 = *(const ulonglong2 *)(fp + ldF), a2 = *(const ulonglong2 *)(fp + 2 * ldF);
                const Fq3 f0 = fq3_make(a0.x, a1.x, a2.x), df = fq3_sub(fq3_make(a0.y, a1.y, a2.y), f0);
                const Fq3Const mc = mu_pow[tb];
                const Fq3 mu = fq3_make(mc.c[0], mc.c[1], mc.c[2]);
                Fq3 f = fq3_add(f0, fq3_mul_small(df, (int)X0));
#pragma unroll
                for (int i = 0; i < SB_XC; i++) {
                    const Fq3 f2 = S3<NU>(f, t.nu);
                    Fq3 prod = f;
                    for (int j = 1; j < B; j++) prod = M3<NU>(prod, fq3_make(fq_sub(f2.c[0], (u64)(j * j)), f2.c[1], f2.c[2]), t.nu);
                    S[i] = fq3_add(S[i], M3<NU>(mu, prod, t.nu));
                    f = fq3_add(f, df);
                }
            }
        } else if (2 * p < n_planes) {
            // round 1: the entries are digits, f(X) a small integer: the norm polynomial runs in the base field, one F_p x F_{p^3} product per table and point
            for (u32 tb = 0; tb < 2 * K * 3; tb++) {
                const u32 side = tb / (3 * K), k = (tb / 3) % K, d = tb % 3;
                const unsigned char *src = (side ? DR : DL) + ((size_t)k * 24 + 8 * d + slot) * ldn + 2 * p;
                const int f0 = sb_digit(src), f1 = 2 * p + 1 < n_planes ? sb_digit(src + 1) : 0;
                if (f0 == 0 && f1 == 0) continue;
                const Fq3Const mc = mu_pow[tb];
                const Fq3 mu = fq3_make(mc.c[0], mc.c[1], mc.c[2]);
                int f = f0 + (int)X0 * (f1 - f0);
#pragma unroll
                for (int i = 0; i < SB_XC; i++) {
                    const u64 fx = fq_from_i64(f), f2 = (u64)((int64_t)f * f);
                    u64 prod = fx;
                    for (int j = 1; j < B; j++) prod = fq_mul(prod, fq_from_i64((int64_t)f2 - j * j));
                    S[i] = fq3_add(S[i], fq3_mul_fq(mu, prod));
                    f += f1 - f0;
                }
            }
        }
        const ulonglong2 b0 = *(const ulonglong2 *)(a.eqB + 2 * p), b1 = *(const ulonglong2 *)(a.eqB + a.ld + 2 * p), b2 = *(const ulonglong2 *)(a.eqB + 2 * a.ld + 2 * p);
        const Fq3 e0 = fq3_make(b0.x, b1.x, b2.x), es = fq3_sub(fq3_make(b0.y, b1.y, b2.y), e0);
        Fq3 e = fq3_add(e0, fq3_mul_small(es, (int)X0));
#pragma unroll
        for (int i = 0; i < SB_XC; i++) {
            acc[i] = fq3_add(acc[i], M3<NU>(S[i], e, t.nu));
            e = fq3_add(e, es);
        }
    }
    u64 vv[3 * SB_XC];
#pragma unroll
    for (int i = 0; i < SB_XC; i++) { vv[3 * i] = acc[i].c[0]; vv[3 * i + 1] = acc[i].c[1]; vv[3 * i + 2] = acc[i].c[2]; }
    __shared__ u64 red[3 * SB_XC];
    block_sum_store<3 * SB_XC>(vv, red);
    __syncthreads();
    if (threadIdx.x < 3 * SB_XC) partial[(size_t)blockIdx.x * nv + (size_t)(X0 + threadIdx.x / 3) * 24 + 3 * slot + threadIdx.x % 3] = red[threadIdx.x];
}
int launch_sb_round(const DevCrt &t, u32 b, const FoldRoundArgs &a, const u64 *F, size_t ldF, const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n_planes,
                    u32 K, const Fq3Const *mu_pow_dev, u64 *partial, u64 *out, hipStream_t s) {
    if (!sb_base_ok(b) || !a.pcnt) return -1;
    u32 gb = (u32)((a.pcnt + 255) / 256);
    if (gb > RED_BLOCKS) gb = RED_BLOCKS;
    const u32 nch = (2 * b + 1 + SB_XC - 1) / SB_XC, nv = nch * SB_XC * 24;
    const dim3 grid(gb, 8, nch), block(256);
#define LF_SB_ROUND(B_)                                                                                                                                        \
    do {                                                                                                                                                       \
        if (F) LF_LAUNCH_SB(B_, true);                                                                                                                         \
        else LF_LAUNCH_SB(B_, false);                                                                                                                          \
    } while (0)
#define LF_LAUNCH_SB(B_, TAB_)                                                                                                                                 \
    do {                                                                                                                                                       \
        if (t.nu2p40) hipLaunchKernelGGL((k_sb_round<true, B_, TAB_>), grid, block, 0, s, t, a, F, ldF, DL, DR, ldn, n_planes, K, mu_pow_dev, partial, nv);    \
        else hipLaunchKernelGGL((k_sb_round<false, B_, TAB_>), grid, block, 0, s, t, a, F, ldF, DL, DR, ldn, n_planes, K, mu_pow_dev, partial, nv);            \
    } while (0)
    if (b == 4) LF_SB_ROUND(4);
    else if (b == 8) LF_SB_ROUND(8);
    else LF_SB_ROUND(16);
#undef LF_LAUNCH_SB
#undef LF_SB_ROUND
    if (sb_launched()) return -1;
    hipLaunchKernelGGL(k_reduce_rows, dim3(nv), dim3(256), 0, s, partial, gb, nv, out);
    return sb_launched();
}

// ---- after r_1: F[(side K + k) 3 + d][3 slot + q][j] = d(2j) + r1 (d(2j+1) - d(2j)), j < m / 2 -----------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sb_materialize(const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n_planes, size_t half, u32 K, Fq3Const r1,
                                                        u64 *F) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u32 slot = blockIdx.y, tb = blockIdx.z;
    if (j >= half) return;
    const u32 side = tb / (3 * K), k = (tb / 3) % K, d = tb % 3;
    const unsigned char *src = (side ? DR : DL) + ((size_t)k * 24 + 8 * d + slot) * ldn + 2 * j;
    const int f0 = 2 * j < n_planes ? sb_digit(src) : 0, f1 = 2 * j + 1 < n_planes ? sb_digit(src + 1) : 0, df = f1 - f0;
    Fq3 v = fq3_mul_small(fq3_make(r1.c[0], r1.c[1], r1.c[2]), df < 0 ? -df : df);
    if (df < 0) v = fq3_neg(v);
    v.c[0] = fq_add(v.c[0], fq_from_i64(f0));
    st3(F + (size_t)tb * 24 * half, half, slot, j, v);
}
int launch_sb_materialize(const DevCrt &, const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n_planes, size_t m, u32 K, Fq3Const r1, u64 *F, hipStream_t s) {
    const size_t half = m / 2;
    if (!half || 2 * K * 3 > 65535) return -1;
    hipLaunchKernelGGL(k_sb_materialize, dim3(cdiv(half, 256), 8, 2 * K * 3), dim3(256), 0, s, DL, DR, ldn, n_planes, half, K, r1, F);
    return sb_launched();
}

// ---- fold of the witnesses: plain int32 convolutions of rho_i in [-32, 32)^24 with the digit vectors, then X^24 = X^12 - 1 ------------------------------------
__global__ void __launch_bounds__(256) k_sb_fold_witness(const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n, u32 K, const int8_t *rho, int32_t *out) {
    extern __shared__ int32_t R[];   // [2K][24]
    for (u32 i = threadIdx.x; i < 2 * K * 24; i += 256) R[i] = rho[i];
    __syncthreads();
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int32_t win[47];
#pragma unroll
    for (int i = 0; i < 47; i++) win[i] = 0;
    for (u32 i = 0; i < 2 * K; i++) {
        const unsigned char *src = (i < K ? DL : DR) + (size_t)(i % K) * 24 * ldn + j;
        const int32_t *r = R + i * 24;
#pragma unroll
        for (int c = 0; c < 24; c++) {
            const int d = sb_digit(src + (size_t)c * ldn);
#pragma unroll
            for (int q = 0; q < 24; q++) win[c + q] += r[q] * d;
        }
    }
    // positions 24 .. 46 fold back top down: X^(24 + i) = X^(12 + i) - X^i
#pragma unroll
    for (int i = 46; i >= 24; i--) { win[i - 12] += win[i]; win[i - 24] -= win[i]; }
#pragma unroll
    for (int c = 0; c < 24; c++) out[(size_t)c * n + j] = win[c];
}
int launch_sb_fold_witness(const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n, u32 K, const int8_t *rho_dev, int32_t *out, hipStream_t s) {
    if (!n || !K) return -1;
    hipLaunchKernelGGL(k_sb_fold_witness, dim3(cdiv(n, 256)), dim3(256), (size_t)2 * K * 24 * 4, s, DL, DR, ldn, n, K, rho_dev, out);
    return sb_launched();
}

}  // namespace lf
