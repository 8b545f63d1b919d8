// bb_kernels_dev.cuh -- device-side helpers shared by the kernel translation units of the BabyBear backend (bb_kernels.hip, bb_rounds.hip): plane-major
// F_{p^9} element access, lazy 96-bit sums of product columns, wave / block reductions, grid helpers, base-2 digits, and BbF, the word policy under which
// bb_kernels.hip instantiates the ring-generic kernels of lf_ring_kernels.cuh.
#pragma once
#include "bb_kernels.h"
#include "lf_ring_kernels.cuh"

namespace lfbb {

using lfk::cdiv;
using lfk::grid_for;

// the device word of this ring for lf_ring_kernels.cuh: centred Montgomery int32, converted at the ABI
struct BbF {
    typedef fe word;
    typedef XbMat9 XbMat;
    static constexpr int RE = lfbb::RE, TAU = lfbb::TAU;
    static constexpr u32 P = BB_P;
    static BB_HD word from_canon(u64 v) { return lfbb::from_canon(v); }
    static BB_HD u32 to_canon(word w) { return lfbb::to_canon(w); }
    static BB_HD word add(word a, word b) { return fadd(a, b); }
    static BB_HD word sub(word a, word b) { return fsub(a, b); }
    static BB_HD word mul(word a, word b) { return fmul(a, b); }
    static BB_HD word one() { return BB_ONE; }
    static BB_HD word from_i64(int64_t v) { return from_small((int32_t)v); }   // |v| < 2^31
    // workload.py splitmix_fq(ring="babybear"): top 32 bits of SplitMix64 word (index+1), mod p
    static __device__ __forceinline__ u64 splitmix(u64 seed, u64 index) {
        u64 z = seed + (index + 1) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z = z ^ (z >> 31);
        return (z >> 32) % BB_P;
    }
    // the 64 x 8 (element, slot) jobs of a relayout tile, two per thread, times the 9 x 9 matrix M (wave-uniform: a kernel argument of centred Montgomery
    // words).  Lane <-> element, as in the plane pass: the odd row length keeps the 32 lanes of a half on distinct banks; wave w takes slots w and w + 4.
    // Column 0 of M is e_0 (ExtBasis::set): a row is eight centred products, 8 H^2 < 2^63, summed in one signed 64-bit register and Montgomery-reduced
    // once -- (M v)~ from M~ and v~.  The row loop stays rolled and serves both jobs of the thread: eight matrix words are live in SGPRs at a time, not
    // all 72 (which spill)
    static __device__ __forceinline__ void xb_slot_pass(fe (*tile)[RE + 1], const XbMat9 &M) {
        fe *p0 = &tile[threadIdx.x % 64][TAU * (threadIdx.x / 64)], *p1 = p0 + TAU * 4;
        fe a[TAU], b[TAU];
#pragma unroll
        for (int j = 0; j < TAU; j++) { a[j] = p0[j]; b[j] = p1[j]; }
#pragma unroll 1
        for (int i = 0; i < TAU; i++) {
            const fe *row = M.m + TAU * i;
            i64 s0 = 0, s1 = 0;
#pragma unroll
            for (int j = 1; j < TAU; j++) { s0 += (i64)row[j] * (i64)a[j]; s1 += (i64)row[j] * (i64)b[j]; }
            const fe r0 = mred(s0), r1 = mred(s1);
            p0[i] = i ? r0 : fadd(r0, a[0]);
            p1[i] = i ? r1 : fadd(r1, b[0]);
        }
    }
};


__device__ __forceinline__ E9 ld9(const fe *tab, size_t ld, u32 slot, size_t i) {
    E9 r;
#pragma unroll
    for (int c = 0; c < TAU; c++) r.c[c] = tab[(size_t)(TAU * slot + c) * ld + i];
    return r;
}
__device__ __forceinline__ void st9(fe *tab, size_t ld, u32 slot, size_t i, const E9 &v) {
#pragma unroll
    for (int c = 0; c < TAU; c++) tab[(size_t)(TAU * slot + c) * ld + i] = v.c[c];
}
__device__ __forceinline__ E9 e9c(const E9C &k) { E9 r; for (int i = 0; i < TAU; i++) r.c[i] = k.c[i]; return r; }
__device__ __forceinline__ E9Pre e9p(const E9PreC &k) { E9Pre r; for (int i = 0; i < TAU; i++) { r.v.c[i] = k.v[i]; r.vn.c[i] = k.vn[i]; } return r; }
// reduce a signed 64-bit sum of residues to a centred word
// |s| <= 9 H^2: two Montgomery steps (s * R^-1, then * R^2 * R^-1) instead of a 64-bit modulo
__device__ __forceinline__ fe fred(i64 s) { return fmul(mred(s), BB_R2C); }

// sum of un-reduced product columns kept as (sum of high halves, sum of low halves); value = Montgomery-reduced total
// (round 4: one signed 96-bit integer in three registers -- add with carry, carry, carry -- instead of two 64-bit sums: three instructions per column instead
// of five and 9 registers less per lazy sum of an F_{p^9} product)
struct HL { u32 a0, a1; int32_t a2; };
__device__ __forceinline__ void hl_zero(HL &a) { a.a0 = 0; a.a1 = 0; a.a2 = 0; }
__device__ __forceinline__ void hl_add(HL &a, i64 T) {
    const u32 t0 = (u32)T, t1 = (u32)((u64)T >> 32);
    const int32_t t2 = (int32_t)t1 >> 31;                     // sign extension word
    asm("v_add_co_u32 %0, vcc, %0, %3\n\tv_addc_co_u32 %1, vcc, %1, %4, vcc\n\tv_addc_co_u32 %2, vcc, %2, %5, vcc"
        : "+v"(a.a0), "+v"(a.a1), "+v"(a.a2)
        : "v"(t0), "v"(t1), "v"(t2)
        : "vcc");
}
// V = a2 2^64 + a1 2^32 + a0 (a2 signed): V 2^-32 mod p = a2 2^32 + a1 + a0 2^-32, centred Montgomery word like mred of the total
__device__ __forceinline__ fe hl_finish(const HL &a) {
    const i64 mid = (i64)a.a1;                                // < 2^32 < 2.2 p
    return fadd(fadd(from_small(a.a2), fred(mid)), mred((i64)a.a0));
}

// ---------------------------------------------------------------------------------------------------------
// the per-element halves of the two transforms, shared by k_crt_fwd / k_icrt_dense (bb_kernels.hip) and the fused product of bb_ring_mul.hip
// coefficients a[72] (Montgomery) -> the 72 NTT words of element j of plane table `out`
__device__ __forceinline__ void crt_store(const fe a[RE], fe *out, size_t ld, size_t j, const DevBb &t) {
#pragma unroll
    for (int r = 0; r < TAU; r++) {
        fe x[8], A[8];
#pragma unroll
        for (int v = 0; v < 8; v++) x[v] = a[r + TAU * v];
        lfk::crt8<BbF>(x, A, t);
#pragma unroll
        for (int p = 0; p < 8; p++) {
            int plane = TAU * t.slot_of_pos[p] + t.pos[r][p];
            out[(size_t)plane * ld + j] = r == 0 ? A[p] : fmul(t.tw[r][p], A[p]);
        }
    }
}
// the dense inverse map of one element: x its 72 NTT words (registers), M the 72 x 72 matrix (LDS in k_icrt_dense, the kernel argument itself -- scalar loads --
// in the fused product) -> the 72 coefficients of element j of plane table `coef`
__device__ __forceinline__ void icrt_dense_elem(const fe *M, const fe (&x)[RE], fe *coef, size_t ld, size_t j) {
    for (int i = 0; i < RE; i++) {
        i64 tot = 0;
#pragma unroll
        for (int g = 0; g < 8; g++) {   // 9 products per exact 64-bit group
            i64 acc = 0;
#pragma unroll
            for (int c = 0; c < 9; c++) acc += (i64)M[i * RE + 9 * g + c] * (i64)x[9 * g + c];
            tot += mred(acc);
        }
        coef[(size_t)i * ld + j] = fred(tot);
    }
}

// ---------------------------------------------------------------------------------------------------------
// reductions: every thread holds NV signed 64-bit partial sums (of centred words)
__device__ __forceinline__ i64 wave_sum(i64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down((long long)v, off, 64);
    return v;
}
template <int NV>
__device__ __forceinline__ void block_sum_store(i64 (&v)[NV], i64 *dst) {
    __shared__ i64 sm[4][NV];
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        i64 s = wave_sum(v[i]);
        if (lane == 0) sm[wave][i] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NV; i += 256) dst[i] = sm[0][i] + sm[1][i] + sm[2][i] + sm[3][i];
}

constexpr u32 RED_BLOCKS = 256;   // partial rows of every two-stage reduction

// bit-plane k of a centred small value: sign(v) * bit_k(|v|)   (base-2 balanced digits, decomposition.rs:159-167)
__device__ __forceinline__ int digit2(int32_t v, u32 k) {
    int32_t m = v < 0 ? -v : v;
    int d = (m >> k) & 1;
    return v < 0 ? -d : d;
}
__device__ __forceinline__ fe fe_from_digit(int d) { return d == 0 ? 0 : (d > 0 ? BB_ONE : -BB_ONE); }

}  // namespace lfbb
