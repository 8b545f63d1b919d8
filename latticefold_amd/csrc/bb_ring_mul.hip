// bb_ring_mul.hip -- the BabyBear instantiation of the ring product kernels (lf_ring_mul.cuh): slots in F_{p^9} = F_p[Y]/(Y^9 - nu), nu from DevBb, centred
// Montgomery int32 words.
//
// Where the reductions sit:
//   NTT form           a product is its nine un-reduced column sums (e9_mul_cols: nine centred products each, |T| <= 9 H^2 < 2^63 -- already the width of the
//                      register, so two products cannot share a signed 64-bit sum).  Each column is added into a signed 96-bit integer (HL, bb_kernels_dev.cuh:
//                      add with carry over three words) and Montgomery-reduced once at the end.  hl_finish takes the top word as a small integer, |a2| < 2^31,
//                      i.e. |sum| < 2^95 = 2^32 columns of 2^63.  FLUSH = 2^30 products (|sum| < 2^93): the sum is finished and restarted there, the parts are
//                      added as centred words.
//   coefficient form   each slot product is reduced (e9_mul: nine Montgomery reductions) and added centred into the 72 accumulator words; the inverse map is nine
//                      products per exact 64-bit group and one reduction per group (icrt_dense_elem), as in k_icrt_dense.
#include "bb_kernels.h"

#include "bb_kernels_dev.cuh"
#include "lf_ring_mul.cuh"
#include "lf_spmv_t.cuh"

namespace lfbb {

struct BbMul {
    typedef fe W;
    typedef DevBb Tab;
    typedef E9 Ext;
    static constexpr int RE = lfbb::RE, TAU = lfbb::TAU;
    static constexpr int COEFF_WAVES = 1;   // the two LDS tiles of a wave (36 KB) allow four waves per CU
    static __device__ __forceinline__ Ext load(const fe *tab, size_t ld, u32 slot, size_t i) { return ld9(tab, ld, slot, i); }
    static __device__ __forceinline__ void store(fe *tab, size_t ld, u32 slot, size_t i, const Ext &v) { st9(tab, ld, slot, i, v); }
    static __device__ __forceinline__ Ext zero() { return e9_zero(); }
    static __device__ __forceinline__ Ext add(const Ext &a, const Ext &b) { return e9_add(a, b); }
    static __device__ __forceinline__ Ext mul(const Ext &a, const Ext &b, const DevBb &t) { return e9_mul(a, b, t.nu); }
    static __device__ __forceinline__ void crt(const fe (&x)[RE], fe *out, size_t ld, size_t j, const DevBb &t) { crt_store(x, out, ld, j, t); }
    static __device__ __forceinline__ void icrt(const fe *M, const fe (&x)[RE], fe *coef, size_t ld, size_t j) { icrt_dense_elem(M, x, coef, ld, j); }

    struct Lazy { HL c[TAU]; };
    static constexpr size_t FLUSH = (size_t)1 << 30;   // |sum| < 2^30 * 2^63 = 2^93 < 2^95 (hl_finish)
    static __device__ __forceinline__ void lazy_zero(Lazy &l) {
#pragma unroll
        for (int c = 0; c < TAU; c++) hl_zero(l.c[c]);
    }
    static __device__ __forceinline__ void mac(Lazy &l, const Ext &a, const Ext &b, const DevBb &t) {
        i64 T[TAU];
        e9_mul_cols(a, b, e9_times_nu(b, t.nu), T);
#pragma unroll
        for (int c = 0; c < TAU; c++) hl_add(l.c[c], T[c]);
    }
    static __device__ __forceinline__ Ext finish(const Lazy &l) {
        E9 r;
#pragma unroll
        for (int c = 0; c < TAU; c++) r.c[c] = hl_finish(l.c[c]);
        return r;
    }
};

void launch_ring_mul_ntt(const DevBb &t, const u64 *a, const u64 *b, size_t n_terms, size_t n, fe *out, hipStream_t s, u32 *flag, const XbMat9 *Ti) {
    lfk::launch_ring_mul_ntt<BbF, BbMul>(t, a, b, n_terms, n, out, s, flag, Ti);
}
void launch_ring_mul_coeff(const DevBb &t, const fe *icrt_mat, const fe *a, const fe *b, size_t n_terms, size_t n, fe *out, hipStream_t s) {
    lfk::launch_ring_mul_coeff<BbMul>(t, icrt_mat, a, b, n_terms, n, out, s);
}
// M^T v for general v (lf_spmv_t.cuh): instantiated here because the lazy sum of slot products is this file's field policy
void launch_spmv_t(const DevBb &t, const u32 *colptr, const u32 *rowidx, const fe *val, const fe *vw, fe *out, size_t n, u32 heavy_min, const u32 *plan,
                   u32 nitems, u32 ncols, fe *part, hipStream_t s) {
    lfk::launch_spmv_t<BbF, BbMul>(t, colptr, rowidx, val, vw, out, n, heavy_min, plan, nitems, ncols, part, s);
}

}  // namespace lfbb
