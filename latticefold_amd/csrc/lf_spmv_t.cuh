// lf_spmv_t.cuh -- out = M^T v for a constraint matrix in CSC form and a vector v of m GENERAL ring elements in NTT form (lf_spmv_t / lf_spmv_t_device), gfx950,
// wave64: out[c] = sum over the entries (r, c) of M of M[r][c] (.) v[r], slot-wise in F_{p^TAU}.  Written once over the word policy F of lf_ring_kernels.cuh
// and the field policy P of lf_ring_mul.cuh (GoldMul<NU2P40> / BbMul: Ext, Lazy, mac, finish, FLUSH), instantiated next to those policies (lf_ring_mul.hip,
// bb_ring_mul.hip).  k_spmv_t_eq, the slot-constant special case of the provers, is not touched.
//
// Operands: colptr / rowidx / val = the CSC arrays of lf_ccs_load (val [nnz][RE] device words, AoS); vw = v element-major in device words [m][RE]
// (launch_aos_words): the eight threads of a column read the RE words of v[r] as one run, as they read the RE words of the non-zero; out = plane table [RE][n].
//
// Two paths, chosen per column by its number of entries against `heavy_min` (SPMV_T_HEAVY unless a test hook of the context says otherwise):
//   light  k_spmv_t: block = 32 columns x 8 slots (the mapping of k_spmv_t_eq: a wave reads the words of eight non-zeros as one run; the sums cross LDS so
//          that the stores are runs of 32 columns per plane).  A thread walks its column alone.  Heavy columns are neither walked nor stored here.
//   heavy  a column of >= heavy_min entries (the constant-1 column of an R1CS holds a row per constraint) would serialise one thread of the light path while
//          the 248 others of its block idle.  The host cuts its CSC range into work items of at most SPMV_T_CHUNK entries (lf_ccs_load: spmv_t_plan);
//          k_spmv_t_heavy runs one block per item, thread = (entry k0 + e + 32 i, slot), 32 entries side by side, reduces the 32 sums of a slot with wave64
//          shuffles (xor 8, 16, 32: lanes of equal slot) and the four waves through LDS, and writes one partial element per item; k_spmv_t_heavy_sum adds
//          the partials of a column (entries / SPMV_T_CHUNK of them) into out.  Items, partials and the output of a column are disjoint from everything
//          the light kernel writes, so the three launches need no order among their stores beyond the stream's.
// Lazy sums: a thread adds its products into one P::Lazy and finishes once; the sum is finished and restarted every P::FLUSH products (the bound in bits
// is stated where the policy defines FLUSH: 2^20 products on Goldilocks with nu = 2^40, 2^30 on BabyBear), the finished parts are added reduced.  The light
// path of a shipped context adds fewer than SPMV_T_HEAVY = 64 products per thread, the heavy path at most SPMV_T_CHUNK / 32 = 16 (static_assert below), so
// the restart runs only where a test hook moved the threshold.  Sums mod p are exact and every stored word is the reduced representative of its residue, so
// the words of out do not depend on the path a column took, nor on the threshold.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lf_ring_kernels.cuh"
#include "lf_spmv_t_plan.h"

namespace lfk {

template <class P>
__device__ __forceinline__ typename P::Ext spmv_t_walk(const typename P::Tab &t, const u32 *rowidx, const typename P::W *val, const typename P::W *vw, size_t k0,
                                                       size_t k1, size_t step, u32 slot) {
    constexpr int RE = P::RE, TAU = P::TAU;
    typename P::Ext acc = P::zero();
    while (k0 < k1) {
        typename P::Lazy l;
        P::lazy_zero(l);
        size_t left = P::FLUSH;
        for (; k0 < k1 && left; k0 += step, left--) {
            const typename P::W *a = val + k0 * RE + TAU * slot, *b = vw + (size_t)rowidx[k0] * RE + TAU * slot;
            typename P::Ext u, v;
#pragma unroll
            for (int q = 0; q < TAU; q++) { u.c[q] = a[q]; v.c[q] = b[q]; }
            P::mac(l, u, v, t);
        }
        acc = P::add(acc, P::finish(l));
    }
    return acc;
}

template <class F, class P>
__global__ void __launch_bounds__(256) k_spmv_t(typename P::Tab t, const u32 *colptr, const u32 *rowidx, const typename P::W *val, const typename P::W *vw,
                                                typename P::W *out, size_t n, u32 heavy_min) {
    constexpr int RE = P::RE, TAU = P::TAU;
    const u32 cl = threadIdx.x >> 3, slot = threadIdx.x & 7;
    const size_t cb = (size_t)blockIdx.x * 32, c = cb + cl;
    __shared__ typename P::W sm[RE][33];
    __shared__ u32 heavy[32];
    typename P::Ext acc = P::zero();
    bool hv = false;
    if (c < n) {
        const size_t k0 = colptr[c], k1 = colptr[c + 1];
        hv = k1 - k0 >= heavy_min;
        if (!hv) acc = spmv_t_walk<P>(t, rowidx, val, vw, k0, k1, 1, slot);
    }
#pragma unroll
    for (int q = 0; q < TAU; q++) sm[TAU * slot + q][cl] = acc.c[q];
    if (slot == 0) heavy[cl] = hv;
    __syncthreads();
    for (u32 o = threadIdx.x; o < RE * 32; o += 256) {
        const u32 row = o >> 5, cc = o & 31;
        if (cb + cc < n && !heavy[cc]) out[(size_t)row * n + cb + cc] = sm[row][cc];
    }
}

template <class T>
__device__ __forceinline__ T shfl_xor_word(T v, int mask) {
    if constexpr (sizeof(T) == 8) return (T)__shfl_xor((unsigned long long)v, mask, 64);
    else return (T)__shfl_xor((int)v, mask, 64);
}
// items [nitems][3] = (column, k0, k1) with k1 - k0 <= SPMV_T_CHUNK; part [nitems][RE]
template <class F, class P>
__global__ void __launch_bounds__(256) k_spmv_t_heavy(typename P::Tab t, const u32 *items, const u32 *rowidx, const typename P::W *val, const typename P::W *vw,
                                                      typename P::W *part) {
    constexpr int RE = P::RE, TAU = P::TAU;
    static_assert(SPMV_T_CHUNK / 32 <= P::FLUSH, "one lazy sum per thread of the heavy path");
    const u32 e = threadIdx.x >> 3, slot = threadIdx.x & 7, wave = threadIdx.x >> 6;
    const size_t k0 = items[3 * (size_t)blockIdx.x + 1], k1 = items[3 * (size_t)blockIdx.x + 2];
    typename P::Ext acc = spmv_t_walk<P>(t, rowidx, val, vw, k0 + e, k1, 32, slot);
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {   // the eight lanes of a wave that hold the same slot
        typename P::Ext o;
#pragma unroll
        for (int q = 0; q < TAU; q++) o.c[q] = shfl_xor_word(acc.c[q], off);
        acc = P::add(acc, o);
    }
    __shared__ typename P::W sm[4][RE];
    if ((threadIdx.x & 63) < 8) {
#pragma unroll
        for (int q = 0; q < TAU; q++) sm[wave][TAU * slot + q] = acc.c[q];
    }
    __syncthreads();
    if (threadIdx.x < RE) {
        const typename P::W s = F::add(F::add(sm[0][threadIdx.x], sm[1][threadIdx.x]), F::add(sm[2][threadIdx.x], sm[3][threadIdx.x]));
        part[(size_t)blockIdx.x * RE + threadIdx.x] = s;
    }
}
// cols [ncols][3] = (column, first item, one past its last item): out[.][column] = the sum of the column's partials
template <class F>
__global__ void __launch_bounds__(256) k_spmv_t_heavy_sum(const u32 *cols, const typename F::word *part, typename F::word *out, size_t n) {
    constexpr int RE = F::RE, G = 256 / RE;
    const u32 c = cols[3 * (size_t)blockIdx.x], p0 = cols[3 * (size_t)blockIdx.x + 1], p1 = cols[3 * (size_t)blockIdx.x + 2];
    const u32 w = threadIdx.x % RE, g = threadIdx.x / RE;
    __shared__ typename F::word sm[G][RE];
    if (g < G) {
        typename F::word s = 0;   // (the zero of either word form)
        for (size_t p = p0 + g; p < p1; p += G) s = F::add(s, part[p * RE + w]);
        sm[g][w] = s;
    }
    __syncthreads();
    if (threadIdx.x < RE) {
        typename F::word s = sm[0][threadIdx.x];
        for (int i = 1; i < G; i++) s = F::add(s, sm[i][threadIdx.x]);
        out[(size_t)threadIdx.x * n + c] = s;
    }
}

// plan (optional): the heavy columns of this matrix on the device, as spmv_t_plan laid them out -- nitems items, then ncols columns; part: nitems * RE words
template <class F, class P>
void launch_spmv_t(const typename P::Tab &t, const u32 *colptr, const u32 *rowidx, const typename P::W *val, const typename P::W *vw, typename P::W *out, size_t n,
                   u32 heavy_min, const u32 *plan, u32 nitems, u32 ncols, typename P::W *part, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL((k_spmv_t<F, P>), dim3(cdiv(n, 32)), dim3(256), 0, s, t, colptr, rowidx, val, vw, out, n, heavy_min);
    if (!nitems) return;
    hipLaunchKernelGGL((k_spmv_t_heavy<F, P>), dim3(nitems), dim3(256), 0, s, t, plan, rowidx, val, vw, part);
    hipLaunchKernelGGL(k_spmv_t_heavy_sum<F>, dim3(ncols), dim3(256), 0, s, plan + 3 * (size_t)nitems, part, out, n);
}

}  // namespace lfk
