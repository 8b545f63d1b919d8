// lfp_check.hip -- gfx950 kernels of the on-device relation checks of the LatticeFold+ slice (lfp_check.cpp; include/lfplus.h lfplus_r1cs_check /
// lfplus_linb_check): R_ComR1CS (r1cs.rs:21-60) and R_LinB (lin.rs:29-40) on the Frog ring Z_p[X]/(X^16 + 1), coefficient form.
//   k_r1cs_residual  (M_A f) o (M_B f) - M_C f row by row, FUSED: the three n x 16 product tables are never written; the only output is the smallest row with a
//                    non-zero residual (one atomicMin per wave that holds one; a satisfied system issues none)
//   k_ccs_residual   the same for a CCS shape (lfplus_ccs_check): sum_i c_i prod_{j in S_i} (M_j f) row by row, fused, the t gathered elements in registers
//   k_linb_dots      one pass over f: up to 8 ring-valued inner products <f, w_t> against SCALAR weight vectors (eq(r_pt), M_j^T eq(r_pt)) and the centred absmax
//   (the centred absmax alone -- the R1CS check, and the LinB check when it runs on tables -- is k_absmax of lfp_digits.hip, which lfplus_linf_norm shares)
// HBM-bound integer work; no MFMA.  Results cross to the host in one download of the result words (lfp_check.cpp).
#include "lfp_kernels.h"
#include "lfp_dev.cuh"

namespace lfp {
static inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }

// coefficient t of (M f)[row] for the 16 lanes of a row group (lane t), canonical.  Constant-coefficient matrices (vals: ONE Montgomery word per non-zero,
// LfpMatrix::valMc): the scalar x element path of k_spmv_ring_const, the whole row as one lazy sum; ring coefficients (16 Montgomery words per non-zero): the
// negacyclic product per non-zero, its 16 signed terms as one lazy sum.  Every lane of the group runs the same trip count (the shuffles stay inside the group).
__device__ __forceinline__ u64 row_gather(const u32 *rowptr, const u32 *col, const u64 *vals, int const_coef, const u64 *x, size_t row, int t) {
    const u32 k0 = rowptr[row], k1 = rowptr[row + 1];
    if (const_coef) {
        Acc160 acc;
        acc160_zero(acc);
        for (u32 k = k0; k < k1; k++) acc160_mad(acc, vals[k], x[(size_t)col[k] * D + t]);
        return acc160_red(acc);
    }
    u64 g = 0;
    for (u32 k = k0; k < k1; k++) {
        const u64 xv = x[(size_t)col[k] * D + t];
        Acc160 acc;
        acc160_bias16(acc);
#pragma unroll
        for (int s = 0; s < D; s++) acc160_mad_signed(acc, vals[(size_t)k * D + s], __shfl(xv, (t - s) & 15, 16), s > t);
        g = add_p(g, acc160_red(acc));
    }
    return g;
}
struct R1csMats {
    const u32 *rowptr[3], *col[3];
    const u64 *vals[3];
    int const_coef[3];
};
// thread = (row, coefficient), 16 rows per block, 4 per wave.  g_A g_B - g_C in Z_p[X]/(X^16 + 1): g_A goes to Montgomery form once, coefficient t of the product is
// the lazy signed sum of its 16 terms (one reduction), g_C is subtracted from the reduced word.  The rows of a wave ascend with the lane index, so the lowest
// lane with a non-zero residual holds the wave's smallest bad row: it alone issues the atomicMin.
__global__ void __launch_bounds__(256) k_r1cs_residual(R1csMats m, const u64 *f, size_t nrows, u64 *first_bad) {
    const size_t row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int t = threadIdx.x & 15;
    bool bad = false;
    if (row < nrows) {      // (the 16 lanes of a row group take this branch together)
        const u64 ga = to_mont(row_gather(m.rowptr[0], m.col[0], m.vals[0], m.const_coef[0], f, row, t));
        const u64 gb = row_gather(m.rowptr[1], m.col[1], m.vals[1], m.const_coef[1], f, row, t);
        const u64 gc = row_gather(m.rowptr[2], m.col[2], m.vals[2], m.const_coef[2], f, row, t);
        Acc160 acc;
        acc160_bias16(acc);
#pragma unroll
        for (int s = 0; s < D; s++) acc160_mad_signed(acc, __shfl(ga, s, 16), __shfl(gb, (t - s) & 15, 16), s > t);
        bad = acc160_red(acc) != gc;
    }
    const unsigned long long mask = __ballot(bad);
    if (mask && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicMin((unsigned long long *)first_bad, (unsigned long long)row);
}
void launch_r1cs_residual(const u32 *const *rowptr, const u32 *const *col, const u64 *const *vals, const int *const_coef, const u64 *f, size_t nrows, u64 *first_bad,
                          hipStream_t s) {
    R1csMats m;
    for (int q = 0; q < 3; q++) { m.rowptr[q] = rowptr[q]; m.col[q] = col[q]; m.vals[q] = vals[q]; m.const_coef[q] = const_coef[q]; }
    hipLaunchKernelGGL(k_r1cs_residual, dim3((unsigned)cdiv(nrows, 16)), dim3(256), 0, s, m, f, nrows, first_bad);
}

// The same for a CCS shape (lfplus_ccs_check): sum_i c_i prod_{j in S_i} (M_j f)[row], FUSED -- the t product tables are never written.  The row's t gathered
// elements stay in registers (selected by unrolled compares: a run-time index would send the array to scratch); a chain's products go through the shuffles of the
// row group as above, a general coefficient (coefM: Montgomery words, read by every lane alike) is the last product of its chain.
struct CcsMats {
    const u32 *rowptr[8], *col[8];
    const u64 *vals[8];
    int const_coef[8];
};
__device__ __forceinline__ u64 ccs_pick(const u64 (&g)[8], u32 j) {
    u64 r = g[0];
#pragma unroll
    for (u32 k = 1; k < 8; k++) r = j == k ? g[k] : r;
    return r;
}
__global__ void __launch_bounds__(256) k_ccs_residual(CcsMats m, CcsDesc d, const u64 *coefM, const u64 *f, size_t nrows, u64 *first_bad) {
    const size_t row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int t = threadIdx.x & 15;
    bool bad = false;
    if (row < nrows) {      // (the 16 lanes of a row group take this branch together)
        u64 g[8];
#pragma unroll
        for (u32 j = 0; j < 8; j++) g[j] = j < d.t ? row_gather(m.rowptr[j], m.col[j], m.vals[j], m.const_coef[j], f, row, t) : 0;
        u64 tot = 0;
        for (u32 i = 0; i < d.q; i++) {
            const u32 lev = d.lev[i];
            if (!lev) continue;
            u64 cur = ccs_pick(g, d.op[i][0]);
            for (u32 l = 1; l < lev; l++) {
                Acc160 acc;
                acc160_bias16(acc);
                if (l < d.len[i]) {
                    const u64 a = to_mont(cur), b = ccs_pick(g, d.op[i][l]);
#pragma unroll
                    for (int s = 0; s < D; s++) acc160_mad_signed(acc, __shfl(a, s, 16), __shfl(b, (t - s) & 15, 16), s > t);
                } else {
#pragma unroll
                    for (int s = 0; s < D; s++) acc160_mad_signed(acc, coefM[i * 16 + s], __shfl(cur, (t - s) & 15, 16), s > t);
                }
                cur = acc160_red(acc);
            }
            const u32 cls = d.cls[i];
            tot = cls == CCS_MINUS_ONE ? sub_p(tot, cur) : cls == CCS_CONST ? add_p(tot, mont_mul(d.cst[i], cur)) : add_p(tot, cur);
        }
        bad = tot != 0;
    }
    const unsigned long long mask = __ballot(bad);
    if (mask && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicMin((unsigned long long *)first_bad, (unsigned long long)row);
}
void launch_ccs_residual(const u32 *const *rowptr, const u32 *const *col, const u64 *const *vals, const int *const_coef, const CcsDesc &d, const u64 *coefM, const u64 *f,
                         size_t nrows, u64 *first_bad, hipStream_t s) {
    CcsMats m;
    for (u32 q = 0; q < 8; q++) {
        const u32 k = q < d.t ? q : 0;      // (unused slots repeat matrix 0: never dereferenced)
        m.rowptr[q] = rowptr[k]; m.col[q] = col[k]; m.vals[q] = vals[k]; m.const_coef[q] = const_coef[k];
    }
    hipLaunchKernelGGL(k_ccs_residual, dim3((unsigned)cdiv(nrows, 16)), dim3(256), 0, s, m, d, coefM, f, nrows, first_bad);
}

// part[chunk][q][16] = sum over the chunk's rows of w[q ldw + row] f[row] for q < NW (w: scalar weights in Montgomery form, f canonical: canonical sums), and the
// centred absmax of f (absmax != nullptr).  thread = (row lane, coefficient) as k_wring: a wave reads 512 contiguous bytes of f per step and the NW weight words of
// its four rows; every product is a lazy term of one of the thread's NW 160-bit sums, reduced once at the end.
template <int NW>
__global__ void __launch_bounds__(256) k_linb_dots(const u64 *f, size_t n, const u64 *w, size_t ldw, u64 *part, u64 *absmax) {
    const u32 c = threadIdx.x & 15, rl = threadIdx.x >> 4;
    Acc160 acc[NW];
#pragma unroll
    for (int q = 0; q < NW; q++) acc160_zero(acc[q]);
    u64 mx = 0;
#pragma unroll 2
    for (size_t row = (size_t)blockIdx.x * 16 + rl; row < n; row += (size_t)gridDim.x * 16) {
        const u64 fv = f[row * D + c];
        const u64 a = abs_centred(fv);
        mx = a > mx ? a : mx;
#pragma unroll
        for (int q = 0; q < NW; q++) acc160_mad(acc[q], w[(size_t)q * ldw + row], fv);
    }
    if (absmax) wave_atomic_max(mx, absmax);
    __shared__ u64 sm[16][NW][16];
#pragma unroll
    for (int q = 0; q < NW; q++) sm[rl][q][c] = acc160_red(acc[q]);
    __syncthreads();
    for (u32 o = threadIdx.x; o < NW * 16; o += 256) {
        u64 t = 0;
        for (int p = 0; p < 16; p++) t = add_p(t, sm[p][o >> 4][o & 15]);
        part[(size_t)blockIdx.x * (NW * 16) + o] = t;
    }
}
// out[q][16] = <f, w_q> for q < nw (nw in {2, 4, 8}); part: eval_chunks(n) * nw * 16 words
void launch_linb_dots(const u64 *f, size_t n, const u64 *w, size_t ldw, u32 nw, u64 *part, u64 *out, u64 *absmax, hipStream_t s) {
    const u32 ch = eval_chunks(n);
    if (nw == 8) hipLaunchKernelGGL((k_linb_dots<8>), dim3(ch), dim3(256), 0, s, f, n, w, ldw, part, absmax);
    else if (nw == 4) hipLaunchKernelGGL((k_linb_dots<4>), dim3(ch), dim3(256), 0, s, f, n, w, ldw, part, absmax);
    else hipLaunchKernelGGL((k_linb_dots<2>), dim3(ch), dim3(256), 0, s, f, n, w, ldw, part, absmax);
    launch_sum_parts(part, ch, (size_t)nw * 16, nw * 16, out, s);
}

}  // namespace lfp
