// lf_ring_mul.hip -- the Goldilocks instantiation of the ring product kernels (lf_ring_mul.cuh): slots in F_{p^3} = F_p[Y]/(Y^3 - nu), canonical u64 words.
// One policy per form of the non-residue, chosen by the launcher from t.nu2p40 as lf_lin_wide.hip and k_lincomb_z do.
//
// Where the reductions sit:
//   NTT form, nu = 2^40   the products of a thread go into one LH5 (lf_field.cuh): five (L, H) column sums of plain signed 64-bit integers, one fold of the
//                         AccP column sums per product (lh5_mac; AccP's carry words hold the wraps of its 64-bit sums: it is used as designed).  Per
//                         product |H| < 2^34 and |L| < 2^33.6; lh5_finish scales H by 2^8 in 64 bits and needs |sum H| < 2^55, i.e. at most 2^21 products.
//                         FLUSH = 2^20 products (|sum H| < 2^54): the sum is finished and restarted there, the parts are added canonically.
//   NTT form, other nu    no deferred sum: each product is reduced (fq3_mul<false>: 128-bit + carry columns, five reductions) and added canonically.
//   coefficient form      each slot product is reduced (fq3_mul<NU>) and added canonically into the 24 accumulator words; the inverse map is acc_mad / acc_reduce
//                         per output coefficient (icrt_dense_elem), as in k_icrt_dense.
#include "lf_kernels.h"

#include "lf_kernels_dev.cuh"
#include "lf_ring_mul.cuh"
#include "lf_spmv_t.cuh"

namespace lf {

template <bool NU>
struct GoldMulBase {
    typedef u64 W;
    typedef DevCrt Tab;
    typedef Fq3 Ext;
    static constexpr int RE = 24, TAU = 3;
    static constexpr int COEFF_WAVES = 2;   // waves per SIMD the fused kernel is compiled for (LDS allows 6 per CU)
    static __device__ __forceinline__ Ext load(const u64 *tab, size_t ld, u32 slot, size_t i) { return ld3(tab, ld, slot, i); }
    static __device__ __forceinline__ void store(u64 *tab, size_t ld, u32 slot, size_t i, Ext v) { st3(tab, ld, slot, i, v); }
    static __device__ __forceinline__ Ext zero() { return fq3_zero(); }
    static __device__ __forceinline__ Ext add(Ext a, Ext b) { return fq3_add(a, b); }
    static __device__ __forceinline__ Ext mul(Ext a, Ext b, const DevCrt &t) { return fq3_mul<NU>(a, b, t.nu); }
    static __device__ __forceinline__ void crt(const u64 (&x)[24], u64 *out, size_t ld, size_t j, const DevCrt &t) { crt_store(x, out, ld, j, t); }
    static __device__ __forceinline__ void icrt(const u64 *M, const u64 (&x)[24], u64 *coef, size_t ld, size_t j) { icrt_dense_elem(M, x, coef, ld, j); }
};
template <bool NU>
struct GoldMul;
template <>
struct GoldMul<true> : GoldMulBase<true> {
    typedef LH5 Lazy;
    static constexpr size_t FLUSH = (size_t)1 << 20;   // |sum H| < 2^20 * 2^34 = 2^54 < 2^55 (lh5_finish)
    static __device__ __forceinline__ void lazy_zero(Lazy &l) { lh5_zero(l); }
    static __device__ __forceinline__ void mac(Lazy &l, Ext a, Ext b, const DevCrt &) { lh5_mac(l, a, b); }
    static __device__ __forceinline__ Ext finish(const Lazy &l) { return lh5_finish(l); }
};
template <>
struct GoldMul<false> : GoldMulBase<false> {
    typedef Fq3 Lazy;   // nothing is deferred
    static constexpr size_t FLUSH = ~(size_t)0;
    static __device__ __forceinline__ void lazy_zero(Lazy &l) { l = fq3_zero(); }
    static __device__ __forceinline__ void mac(Lazy &l, Ext a, Ext b, const DevCrt &t) { l = fq3_add(l, fq3_mul<false>(a, b, t.nu)); }
    static __device__ __forceinline__ Ext finish(const Lazy &l) { return l; }
};

void launch_ring_mul_ntt(const DevCrt &t, const u64 *a, const u64 *b, size_t n_terms, size_t n, u64 *out, hipStream_t s, u32 *flag, const XbMat3 *Ti) {
    if (t.nu2p40) lfk::launch_ring_mul_ntt<GoldF, GoldMul<true>>(t, a, b, n_terms, n, out, s, flag, Ti);
    else lfk::launch_ring_mul_ntt<GoldF, GoldMul<false>>(t, a, b, n_terms, n, out, s, flag, Ti);
}
void launch_ring_mul_coeff(const DevCrt &t, const u64 *icrt_mat, const u64 *a, const u64 *b, size_t n_terms, size_t n, u64 *out, hipStream_t s) {
    if (t.nu2p40) lfk::launch_ring_mul_coeff<GoldMul<true>>(t, icrt_mat, a, b, n_terms, n, out, s);
    else lfk::launch_ring_mul_coeff<GoldMul<false>>(t, icrt_mat, a, b, n_terms, n, out, s);
}
// M^T v for general v (lf_spmv_t.cuh): instantiated here because the lazy sum of slot products is this file's field policy
void launch_spmv_t(const DevCrt &t, const u32 *colptr, const u32 *rowidx, const u64 *val, const u64 *vw, u64 *out, size_t n, u32 heavy_min, const u32 *plan,
                   u32 nitems, u32 ncols, u64 *part, hipStream_t s) {
    if (t.nu2p40) lfk::launch_spmv_t<GoldF, GoldMul<true>>(t, colptr, rowidx, val, vw, out, n, heavy_min, plan, nitems, ncols, part, s);
    else lfk::launch_spmv_t<GoldF, GoldMul<false>>(t, colptr, rowidx, val, vw, out, n, heavy_min, plan, nitems, ncols, part, s);
}

}  // namespace lf
