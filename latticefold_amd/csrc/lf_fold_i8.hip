// lf_fold_i8.hip -- compute_f_0 (folding.rs:258-268) on the int8 matrix cores (gfx950 v_mfma_i32_16x16x64_i8), K <= 16 bit-planes:
//     f_0[c][j] = sum_{side, k, a} W[c][(side, a, k)] * digit_k(planes_side[a][j])            (digit_k(v) = sign(v) bit_k(|v|))
// was k_fold_witness<4>: per column 24 coefficients x 2 sides x 4 nibbles of 24-word LDS rows -- 18 KB of LDS reads per column, LDS-bound.
//
// The product of the bit-planes with the short challenges rho_{side,k} is a convolution: the unwrapped coefficient p < 47 is
// u[p] = sum rho_{side,k}[p - a] digit_k(v_a), and X^24 = X^12 - 1 (so X^36 = -1) folds it to
//     f_0[c] = u[c] - u[c + 24] - u[c + 36]   (c < 12),        f_0[c] = u[c] + u[c + 12]   (12 <= c < 24).
// The wrap is built INTO the matrix: W[c][a] = rho[c - a] - rho[c + 24 - a] - rho[c + 36 - a] resp. rho[c - a] + rho[c + 12 - a] (terms with an index outside
// 0 .. 23 are absent).  For a given (c, a) at most two of the terms exist (c - a >= 0 excludes c + 24 - a <= 23), so |W| <= 2 max|rho|: the launcher is
// handed max|rho| by the host, which has the coefficients, and declines above 63 (a short challenge has coefficients in [-32, 32): |W| <= 64).  The
// accumulators are the int32 coefficients themselves: |f_0[c]| <= 768 * 126, no recombination.
//
// GEMM shape per wave: M = 24 rows c (two row tiles, the second half empty), inner dimension 2 * 24 * 16 = 768 = 12 K-steps in the order (side, a, k)
// with k fastest -- the 16 inner positions of lane group g in K-step s are the 16 digits of ONE plane entry, (side, a) = 4 s + g, cut in registers --,
// columns = 64 witness columns as four column tiles: tile t holds the columns 4 n + t (n = lane & 15), so a lane loads the entries of its four tiles with
// one 16-byte load (a lane group reads 256 contiguous bytes of a plane row) and stores the four results of a row the same way.
// A and B meet position by position inside a lane group, so the hardware's order of the inner positions does not matter.
#include <hip/hip_runtime.h>
#include "lf_field.cuh"
#include "lf_kernels.h"
#include "lf_i8_mma.cuh"

namespace lf {
using namespace i8mma;

// four bits of x (bit b -> byte b) times mul (1, or 0xFF for a negative entry: bytes 0x01 -> 0xFF = -1).  x * 0x00204081 copies bit b to the positions
// b + 7 j, all distinct for b < 4, j < 4 (no carries); the mask keeps b + 7 b = 8 b.
__device__ __forceinline__ int fwi_spread(u32 x, u32 mul) { return (int)((((x & 15u) * 0x00204081u) & 0x01010101u) * mul); }
__device__ __forceinline__ v4i fwi_digits(int32_t v) {
    const u32 m = (u32)(v < 0 ? -v : v), mul = v < 0 ? 0xFFu : 1u;
    return v4i{fwi_spread(m, mul), fwi_spread(m >> 4, mul), fwi_spread(m >> 8, mul), fwi_spread(m >> 12, mul)};
}

// wave = 64 columns at a time; the block's A operands (W in operand order, [row tile][K-step][lane] x 16 bytes: 24 KB) are built once per block in LDS
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_fold_witness_i8(const int32_t *planesL, const int32_t *planesR, size_t n, u32 K, const int8_t *rho, int32_t *out) {
    __shared__ int8_t rh[2 * 16 * 24];
    __shared__ __align__(16) int As[2 * 12 * 64 * 4];
    for (u32 i = threadIdx.x; i < 2 * 16 * 24; i += 256) {
        const u32 a = i % 24, k = (i / 24) % 16, side = i / (24 * 16);
        rh[i] = k < K ? rho[(size_t)(side * K + k) * 24 + a] : (int8_t)0;
    }
    __syncthreads();
    // word w of lane (m, g) at (row tile mt, K-step s): the bytes k = 4 w .. 4 w + 3 of row c = 16 mt + m against (side, a) = 4 s + g
    for (u32 i = threadIdx.x; i < 2 * 12 * 64 * 4; i += 256) {
        const u32 w = i & 3, ln = (i >> 2) & 63, s = (i >> 8) % 12, mt = i / (12 * 256);
        const int c = 16 * (int)mt + (int)(ln & 15);
        const u32 sa = 4 * s + (ln >> 4), side = sa / 24;
        const int a = (int)(sa % 24);
        u32 word = 0;
        if (c < 24) {
#pragma unroll
            for (u32 b = 0; b < 4; b++) {
                const int8_t *r = rh + (side * 16 + 4 * w + b) * 24;
                auto at = [&](int idx) { return (idx >= 0 && idx < 24) ? (int)r[idx] : 0; };
                const int val = c < 12 ? at(c - a) - at(c + 24 - a) - at(c + 36 - a) : at(c - a) + at(c + 12 - a);
                word |= ((u32)val & 0xFFu) << (8 * b);
            }
        }
        As[i] = (int)word;
    }
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nn = lane & 15, g = lane >> 4;
    const size_t chunks = (n + 63) / 64;
    for (size_t ch = (size_t)blockIdx.x * 4 + wave; ch < chunks; ch += (size_t)gridDim.x * 4) {
        const size_t col = ch * 64 + 4 * nn;      // n is a multiple of 4 (launcher): a lane's four columns are all inside or all outside
        const bool live = col < n;
        const size_t lcol = live ? col : 0;       // (a lane beyond the last column reads columns 0 .. 3: its tile columns are its own, and it stores nothing)
        int4 v[12];
#pragma unroll
        for (int s = 0; s < 12; s++) {
            const int32_t *row = (s < 6 ? planesL : planesR) + (size_t)(4 * (s % 6) + g) * n;   // (side, a) = 4 s + g: the K-steps 0 .. 5 are the left side's
            v[s] = *(const int4 *)(row + lcol);
        }
        v4i acc[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int t = 0; t < 4; t++) acc[mt][t] = v4i{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 12; s++) {
            const v4i a0 = *(const v4i *)(As + ((0 * 12 + s) * 64 + lane) * 4), a1 = *(const v4i *)(As + ((1 * 12 + s) * 64 + lane) * 4);
            const int32_t e[4] = {v[s].x, v[s].y, v[s].z, v[s].w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const v4i b = fwi_digits(e[t]);
                acc[0][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc[1][t], 0, 0, 0);
            }
            // (the digits of a K-step are cut when it runs: moved ahead of the earlier steps' MFMAs, the 12 x 4 x 4 digit words do not fit next to the plane entries)
            __builtin_amdgcn_sched_barrier(0);
        }
        // register r of tile t: row c = 16 mt + 4 g + r, column 4 nn + t
        if (live) {
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const u32 c = 16 * mt + 4 * g + r;
                    if (c < 24) *(int4 *)(out + (size_t)c * n + col) = int4{acc[mt][0][r], acc[mt][1][r], acc[mt][2][r], acc[mt][3][r]};
                }
        }
    }
}

// Result: lf_i8_launch.h (shape not handled: the caller launches k_fold_witness)
int launch_fold_witness_i8(const int32_t *planesL, const int32_t *planesR, size_t n, u32 K, const int8_t *rho_dev, int rho_max, int32_t *out, hipStream_t s) {
    if (K < 1 || K > 16 || n == 0 || (n & 3) || rho_max > 63) return I8_ERR_SHAPE;
    if ((((uintptr_t)planesL) | ((uintptr_t)planesR) | ((uintptr_t)out)) & 15) return I8_ERR_SHAPE;
    const size_t blocks = (n + 255) / 256;       // four chunks of 64 columns per block and trip
    hipLaunchKernelGGL(k_fold_witness_i8, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, planesL, planesR, n, K, rho_dev, out);
    return i8_launched();
}
}  // namespace lf
