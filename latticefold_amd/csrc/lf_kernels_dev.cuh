// lf_kernels_dev.cuh -- device-side helpers shared by the kernel translation units of the Goldilocks backend (lf_kernels.hip, lf_rounds.hip): the F_{p^3}
// product wrappers, the nu-specialised launch macro, grid helpers, wave / block reductions, plane-major element access, base-2 digits, and GoldF, the word
// policy under which lf_kernels.hip instantiates the ring-generic kernels of lf_ring_kernels.cuh.
#pragma once
#include <stddef.h>

#include "lf_kernels.h"
#include "lf_ring_kernels.cuh"

namespace lf {

#define NUARG t.nu
template <bool NU> __device__ __forceinline__ Fq3 M3(Fq3 a, Fq3 b, u64 nu) { return fq3_mul<NU>(a, b, nu); }
template <bool NU> __device__ __forceinline__ Fq3 S3(Fq3 a, u64 nu) { return fq3_sqr<NU>(a, nu); }

#define LF_LAUNCH(KERNEL, nuflag, grid, block, stream, ...)                                   \
    do {                                                                                      \
        if (nuflag) hipLaunchKernelGGL((KERNEL<true>), grid, block, 0, stream, __VA_ARGS__);  \
        else hipLaunchKernelGGL((KERNEL<false>), grid, block, 0, stream, __VA_ARGS__);        \
    } while (0)

using lfk::cdiv;
using lfk::grid_for;

// the device word of this ring for lf_ring_kernels.cuh: canonical u64, so both conversions are the identity
struct GoldF {
    typedef u64 word;
    typedef XbMat3 XbMat;
    static constexpr int RE = 24, TAU = 3;
    static constexpr u64 P = LF_P;
    static LF_HD word from_canon(u64 v) { return v; }
    static LF_HD u64 to_canon(word w) { return w; }
    static LF_HD word add(word a, word b) { return fq_add(a, b); }
    static LF_HD word sub(word a, word b) { return fq_sub(a, b); }
    static LF_HD word mul(word a, word b) { return fq_mul(a, b); }
    static LF_HD word one() { return 1; }
    static LF_HD word from_i64(int64_t v) { return fq_from_i64(v); }
    // workload.py splitmix_fq: SplitMix64 word (index + 1), minus p if not below it
    static __device__ __forceinline__ u64 splitmix(u64 seed, u64 index) {
        u64 z = seed + (index + 1) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z = z ^ (z >> 31);
        return z >= LF_P ? z - LF_P : z;
    }
    // the 64 x 8 (element, slot) jobs of a relayout tile, two per thread, times the 3 x 3 matrix M (wave-uniform: a kernel argument, held in SGPRs).  Lane <->
    // element, as in the plane pass: the odd row length keeps the 64-bit LDS accesses of a 32-lane half on distinct banks.  Column 0 of M is e_0 (ExtBasis::set),
    // so a slot costs six products; two products of words < 2^64 and their carry fit the 128-bit + carry accumulator, whatever the words are
    static __device__ __forceinline__ void xb_slot_pass(u64 (*tile)[RE + 1], const XbMat3 &M) {
        for (int idx = threadIdx.x; idx < 64 * 8; idx += 256) {
            u64 *v = &tile[idx % 64][3 * (idx / 64)];
            const u64 v0 = fq_canon(v[0]), v1 = v[1], v2 = v[2];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                Acc s;
                acc_set(s, M.m[3 * i + 1], v1);
                acc_mad(s, M.m[3 * i + 2], v2);
                const u64 r = acc_reduce(s);
                v[i] = i ? r : fq_add(r, v0);
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------
// reductions
__device__ __forceinline__ u64 wave_sum_fq(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        u64 o = __shfl_down((unsigned long long)v, off, 64);
        v = fq_add(v, o);
    }
    return v;
}
// sum `v[0..NV)` over the 256 threads of the block, write to dst[0..NV) (thread-0-side); values canonical
template <int NV>
__device__ __forceinline__ void block_sum_store(u64 (&v)[NV], u64 *dst) {
    __shared__ u64 sm[4][NV];
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        u64 s = wave_sum_fq(v[i]);
        if (lane == 0) sm[wave][i] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NV; i += 256) dst[i] = fq_add(fq_add(sm[0][i], sm[1][i]), fq_add(sm[2][i], sm[3][i]));
}

__device__ __forceinline__ u64 fq_from_digit(int d) { return d == 0 ? 0 : (d > 0 ? 1 : LF_P - 1); }

// bit-plane k of a centred small value: sign(v) * bit_k(|v|)   (base-2 balanced digits, decomposition.rs:159-167)
__device__ __forceinline__ int digit2(int32_t v, u32 k) {
    int32_t m = v < 0 ? -v : v;
    int d = (m >> k) & 1;
    return v < 0 ? -d : d;
}

__device__ __forceinline__ Fq3 ld3(const u64 *tab, size_t ld, u32 slot, size_t i) {
    return fq3_make(tab[(size_t)(3 * slot) * ld + i], tab[(size_t)(3 * slot + 1) * ld + i], tab[(size_t)(3 * slot + 2) * ld + i]);
}
__device__ __forceinline__ void st3(u64 *tab, size_t ld, u32 slot, size_t i, Fq3 v) {
    tab[(size_t)(3 * slot) * ld + i] = v.c[0]; tab[(size_t)(3 * slot + 1) * ld + i] = v.c[1]; tab[(size_t)(3 * slot + 2) * ld + i] = v.c[2];
}

// ---------------------------------------------------------------------------------------------------------
// the per-element halves of the two transforms, shared by k_crt_fwd / k_icrt_dense (lf_kernels.hip) and the fused product of lf_ring_mul.hip
// coefficients a[24] (canonical) -> stores the 24 NTT words of element j into plane table `out` (ld = n)
__device__ __forceinline__ void crt_store(const u64 a[24], u64 *out, size_t ld, size_t j, const DevCrt &t) {
    u64 x[8], A0[8], A1[8], A2[8];
#pragma unroll
    for (int v = 0; v < 8; v++) x[v] = a[3 * v];
    lfk::crt8<GoldF>(x, A0, t);
#pragma unroll
    for (int v = 0; v < 8; v++) x[v] = a[3 * v + 1];
    lfk::crt8<GoldF>(x, A1, t);
#pragma unroll
    for (int v = 0; v < 8; v++) x[v] = a[3 * v + 2];
    lfk::crt8<GoldF>(x, A2, t);
#pragma unroll
    for (int p = 0; p < 8; p++) {
        int s3 = 3 * t.slot_of_pos[p];
        out[(size_t)s3 * ld + j] = A0[p];
        out[(size_t)(s3 + t.pos1[p]) * ld + j] = fq_mul(t.tw1[p], A1[p]);
        out[(size_t)(s3 + t.pos2[p]) * ld + j] = fq_mul(t.tw2[p], A2[p]);
    }
}
// the dense inverse map of one element: x its 24 NTT words (registers), M the 24 x 24 matrix (LDS in k_icrt_dense, the kernel argument itself -- scalar loads --
// in the fused product) -> the 24 coefficients of element j of plane table `coef`
__device__ __forceinline__ void icrt_dense_elem(const u64 *M, const u64 (&x)[24], u64 *coef, size_t ld, size_t j) {
    for (int i = 0; i < 24; i++) {
        Acc a;
        acc_set(a, M[i * 24], x[0]);
#pragma unroll
        for (int c = 1; c < 24; c++) acc_mad(a, M[i * 24 + c], x[c]);
        coef[(size_t)i * ld + j] = acc_reduce(a);
    }
}

constexpr u32 RED_BLOCKS = 256;   // partial rows of every two-stage reduction

// fused fix_variables of the linearization round kernels (k_lin_round, k_lin_round_wide): the challenge and where the fixed tables go
struct LinFix { Fq3Const r; u64 *mzo; size_t ldo; u64 *eqo; size_t ldeo; };
// c_i[3 slot ..] of the by-value descriptor, read from the kernel-argument segment itself (constant memory; the descriptor is the second argument of every
// kernel that takes it, behind DevCrt)
__device__ __forceinline__ const u64 *lin_desc_coef(const LinCombDesc &, u32 i, u32 slot) {
    constexpr size_t off = (sizeof(DevCrt) + alignof(LinCombDesc) - 1) / alignof(LinCombDesc) * alignof(LinCombDesc);
    const char *ka = (const char *)__builtin_amdgcn_kernarg_segment_ptr();
    return (const u64 *)(ka + off + offsetof(LinCombDesc, c)) + (size_t)i * 24 + 3 * slot;
}

// out[i] = sum_b partial[b*nv + i]; one block per i
static __global__ void __launch_bounds__(256) k_reduce_rows(const u64 *partial, u32 nblocks, u32 nv, u64 *out) {
    u32 i = blockIdx.x;
    u64 acc[1] = {0};
    for (u32 b = threadIdx.x; b < nblocks; b += 256) acc[0] = fq_add(acc[0], partial[(size_t)b * nv + i]);
    block_sum_store<1>(acc, out + i);
}

}  // namespace lf
