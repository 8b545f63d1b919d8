// lf_ring_mul.cuh -- the product of two arrays of ring elements (lf_ring_mul / lf_ring_mul_device), gfx950, wave64: out[x] = sum_{i < n_terms} a_i[x] * b_i[x].
// Two kernels, each written ONCE over the word policy F of lf_ring_kernels.cuh and a field policy P: the rings' bodies differ in the field calls alone.  The
// policies are the rings' own (lf_ring_mul.hip: GoldMul<NU2P40>, bb_ring_mul.hip: BbMul); this header includes no ring header.
//
// The field policy:
//   W, Tab, RE, TAU         device word, the ring's table struct (kernel argument, by value), words per element, extension degree of a slot
//   Ext, load, store        an element of F_{p^TAU} in registers (words c[TAU]); slot `slot` of element i of a plane table (global or LDS)
//   zero, add, mul          reduced arithmetic of Ext (mul: one product, reduced)
//   Lazy, lazy_zero, mac, finish, FLUSH
//                           a sum of products whose reduction is deferred: mac adds one product, finish reduces; FLUSH is the number of products after which the
//                           kernel finishes the sum and starts a new one.  The policy states the bound in bits that FLUSH comes from
//   COEFF_WAVES             waves per SIMD k_ring_mul_coeff is compiled for
//   crt, icrt               the per-element halves of the ring's transforms (crt_store / icrt_dense_elem of the ring's *_kernels_dev.cuh)
//
// k_ring_mul_ntt   NTT form: AoS operands in, the resident plane layout [RE][n] out.  The relayout of the operands is IN the kernel: a block stages 64 elements
//                  of a_i and of b_i through two LDS tiles exactly as k_aos_to_soa does (coalesced AoS reads, the canonical test of a caller's own words, the
//                  external-basis pass F::xb_slot_pass in the tile), a thread owns slots s and s + 4 of one element (the job map of xb_slot_pass: lane <->
//                  element, odd row length), accumulates over the terms and writes its 2 TAU reduced words to the planes, lane <-> consecutive element.  A call
//                  moves 2 n_terms + 1 tables here and two more in the relayout out (which keeps the output behind the canonical-word flag); with the operands
//                  relayouted by k_aos_to_soa first it moved 4 n_terms + 1 + 2 -- measured at 2^20 elements, one term: 1.5 x one lf_ntt_fwd_dev, both rings.
//                  Exact for ANY n_terms: the lazy sum is finished every FLUSH terms, the finished parts are added reduced.
// k_ring_mul_coeff coefficient form, fused, on plane tables [RE][n] (table i at a + i * RE * n; the operands come through k_aos_to_soa).  A thread owns one
//                  element: per term it reads the RE coefficients of a_i[x] and of b_i[x], transforms both (P::crt) into its own columns of two LDS tiles
//                  [RE][64] (the transform stores by a table-driven plane index, which registers cannot take), multiplies slot by slot and adds the reduced
//                  products into RE accumulator words in registers; ONE inverse transform (P::icrt, the dense map, its matrix read through uniform scalar
//                  loads of the kernel argument) per element whatever n_terms is.  Nothing in NTT form goes to HBM.  No reduction is deferred across terms
//                  (the accumulator is RE reduced words), so there is nothing to bound.  A column of either tile is written and read by one thread only:
//                  no barrier.  Block = one wave: 24.0 KB (Goldilocks) / 36.0 KB (BabyBear) of LDS.  (Reading the AoS operands through LDS tiles here
//                  too, as k_ring_mul_ntt does, was built and measured at 2^20 elements: Goldilocks unchanged, BabyBear 3.5 -> 4.9 ms; not kept.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lf_ring_kernels.cuh"

namespace lfk {

template <class F, class P, bool CHECKED, bool XBASIS, class... Opt>
__global__ void __launch_bounds__(256) k_ring_mul_ntt(typename P::Tab t, const u64 *a, const u64 *b, size_t n_terms, size_t n, typename F::word *out, Opt... opt) {
    static_assert(sizeof...(Opt) == (CHECKED ? 1 : 0) + (XBASIS ? 1 : 0), "flag if CHECKED, matrix if XBASIS");
    typedef typename F::word W;
    constexpr int RE = F::RE, TAU = F::TAU;
    __shared__ W ta[64][RE + 1], tb[64][RE + 1];
    const size_t base = (size_t)blockIdx.x * 64;
    const int e = threadIdx.x % 64, s0 = threadIdx.x / 64;   // this thread: slots s0 and s0 + 4 of element base + e
    bool bad = false;
    typename P::Ext r0 = P::zero(), r1 = P::zero();
    for (size_t k0 = 0; k0 < n_terms;) {
        const size_t k1 = n_terms - k0 > P::FLUSH ? k0 + P::FLUSH : n_terms;
        typename P::Lazy l0, l1;
        P::lazy_zero(l0);
        P::lazy_zero(l1);
        for (size_t k = k0; k < k1; k++) {
            const u64 *ak = a + k * n * RE, *bk = b + k * n * RE;
            for (int idx = threadIdx.x; idx < 64 * RE; idx += 256) {
                const size_t el = base + idx / RE;
                const u64 va = el < n ? ak[el * RE + idx % RE] : 0, vb = el < n ? bk[el * RE + idx % RE] : 0;
                if (CHECKED) bad |= va >= F::P || vb >= F::P;
                ta[idx / RE][idx % RE] = F::from_canon(va);
                tb[idx / RE][idx % RE] = F::from_canon(vb);
            }
            __syncthreads();
            if constexpr (XBASIS) {
                const typename F::XbMat &M = opt_arg<typename F::XbMat>(opt...);
                F::xb_slot_pass(ta, M);
                F::xb_slot_pass(tb, M);
                __syncthreads();
            }
            typename P::Ext u0, v0, u1, v1;
#pragma unroll
            for (int q = 0; q < TAU; q++) {
                u0.c[q] = ta[e][TAU * s0 + q]; v0.c[q] = tb[e][TAU * s0 + q];
                u1.c[q] = ta[e][TAU * (s0 + 4) + q]; v1.c[q] = tb[e][TAU * (s0 + 4) + q];
            }
            P::mac(l0, u0, v0, t);
            P::mac(l1, u1, v1, t);
            __syncthreads();   // (the tiles are free for the next term)
        }
        r0 = P::add(r0, P::finish(l0));
        r1 = P::add(r1, P::finish(l1));
        k0 = k1;
    }
    if constexpr (CHECKED) {
        if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(opt_arg<uint32_t *>(opt...), 1u);   // (every thread ran the same trips: whole waves vote)
    }
    if (base + e < n) {
        P::store(out, n, s0, base + e, r0);
        P::store(out, n, s0 + 4, base + e, r1);
    }
}

constexpr int RING_MUL_COEFF_BLOCK = 64;
template <class P>
__global__ void __launch_bounds__(RING_MUL_COEFF_BLOCK, P::COEFF_WAVES) k_ring_mul_coeff(typename P::Tab t, const typename P::W *mat, const typename P::W *a,
                                                                                          const typename P::W *b, size_t n_terms, size_t n, typename P::W *out) {
    typedef typename P::W W;
    constexpr int RE = P::RE, TAU = P::TAU, B = RING_MUL_COEFF_BLOCK;
    __shared__ W sa[RE * B], sb[RE * B];
    const uint32_t lane = threadIdx.x;
    const size_t j = (size_t)blockIdx.x * B + lane;
    if (j >= n) return;
    const size_t tab = (size_t)RE * n;
    W acc[RE];
#pragma unroll
    for (int c = 0; c < RE; c++) acc[c] = 0;   // (the zero of either word form)
#pragma unroll 1
    for (size_t k = 0; k < n_terms; k++) {
        {
            W x[RE];
#pragma unroll
            for (int c = 0; c < RE; c++) x[c] = a[k * tab + (size_t)c * n + j];
            P::crt(x, sa, B, lane, t);
        }
        __builtin_amdgcn_sched_barrier(0);   // (the scheduler would hoist the loads of b, and below of all eight slots, over everything before them: 256 registers)
        {
            W x[RE];
#pragma unroll
            for (int c = 0; c < RE; c++) x[c] = b[k * tab + (size_t)c * n + j];
            P::crt(x, sb, B, lane, t);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < RE / TAU; s++) {
            typename P::Ext u = P::load(sa, B, s, lane), v = P::load(sb, B, s, lane), w, pr = P::mul(u, v, t);
#pragma unroll
            for (int q = 0; q < TAU; q++) w.c[q] = acc[TAU * s + q];
            w = P::add(w, pr);
#pragma unroll
            for (int q = 0; q < TAU; q++) acc[TAU * s + q] = w.c[q];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    P::icrt(mat, acc, out, n, j);
}

// a, b: the caller's (or the staged) AoS arrays of canonical words; flag: the checked form; Ti: T^-1 of a context in an external basis
template <class F, class P>
void launch_ring_mul_ntt(const typename P::Tab &t, const u64 *a, const u64 *b, size_t n_terms, size_t n, typename F::word *out, hipStream_t s, uint32_t *flag,
                         const typename F::XbMat *Ti) {
    if (!n) return;
    const dim3 g(cdiv(n, 64)), bl(256);
    if (flag && Ti) hipLaunchKernelGGL((k_ring_mul_ntt<F, P, true, true>), g, bl, 0, s, t, a, b, n_terms, n, out, flag, *Ti);
    else if (flag) hipLaunchKernelGGL((k_ring_mul_ntt<F, P, true, false>), g, bl, 0, s, t, a, b, n_terms, n, out, flag);
    else if (Ti) hipLaunchKernelGGL((k_ring_mul_ntt<F, P, false, true>), g, bl, 0, s, t, a, b, n_terms, n, out, *Ti);
    else hipLaunchKernelGGL((k_ring_mul_ntt<F, P, false, false>), g, bl, 0, s, t, a, b, n_terms, n, out);
}
template <class P>
void launch_ring_mul_coeff(const typename P::Tab &t, const typename P::W *mat, const typename P::W *a, const typename P::W *b, size_t n_terms, size_t n,
                           typename P::W *out, hipStream_t s) {
    constexpr int B = RING_MUL_COEFF_BLOCK;
    if (n) hipLaunchKernelGGL(k_ring_mul_coeff<P>, dim3(cdiv(n, B)), dim3(B), 0, s, t, mat, a, b, n_terms, n, out);
}

}  // namespace lfk
