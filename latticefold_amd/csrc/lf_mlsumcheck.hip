// lf_mlsumcheck.hip -- the round kernel of the generic sumcheck (lf_mlsumcheck_*; MLSumcheck::prove_as_subprotocol, utils/sumcheck/prover.rs:56-162), gfx950,
// wave64: the round polynomial of  g = sum_i coef_i prod_k T_{idx[k]}  at X = 0 .. degree, written ONCE over a field policy P and instantiated for Goldilocks
// (slots in F_{p^3}, canonical u64 words) and BabyBear (slots in F_{p^9}, centred Montgomery int32 words).
//
// Mapping: thread = (pair, slot).  slot = blockIdx.y, so a wave sums over pairs alone; blockIdx.x strides over the pairs (at most lfml::MAX_BLOCKS blocks);
// blockIdx.z is the point group: points [PTS z, PTS z + PTS) of the degree + 1, PTS a compile-time constant of the ring.  The same code serves degree 1 and
// degree 8; a point past the degree in the last group is computed and not stored.
//
// Per pair, per term (prover.rs:111-143, literally: value, step, repeated addition, product at each point, sum): the factors are walked ONE AT A TIME -- load
// (v0, v1) of the factor, step = v1 - v0, the value at the group's first point by repeated addition (the step is an addition, never a product), then one
// product per point into the PTS running products `pr`.  There is no per-table array and no run-time index into registers: pr[] and acc[] are indexed by
// unrolled compile-time loops only.  The term's product is scaled by its coefficient in this slot -- class COEF_GENERAL: one more product; +1 / -1: an
// addition / subtraction; 0: the term is skipped in this slot before anything is loaded -- and added to the PTS sums `acc`.
//
// Every product is reduced and every sum is a reduced field addition: NOTHING is deferred, so no accumulator has a bound to respect and there is no flush
// (the kernel reads 2 q' TAU words per pair and multiplies PTS q' times on them, q' = factors in all terms: on the linearization shape it is bound by the
// products, and a deferred sum would save one reduction in |S_i| + 1).
//
// The descriptor (offsets, indices, coefficient classes) is the first kernel argument and is read from the kernel-argument segment: wave-uniform scalar loads,
// no indexed by-value struct (which goes to scratch).  The coefficient words are read from the context's buffer with a wave-uniform address, once per term.
//
// Reduction over pairs: wave64 shuffle reduction, four wave sums through LDS, one partial row per block ([block][point][slot][TAU], the message's own order),
// finished by k_mls_finish (the k_reduce_rows pattern of the linearization rounds), which writes canonical words.
//
// Resource usage of the cross-compile (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage) is recorded in DESIGN.md section 8c: no scratch on
// either ring.
#include "lf_mlsumcheck.h"

#include "bb_kernels.h"
#include "lf_kernels.h"

#include "bb_kernels_dev.cuh"
#include "lf_kernels_dev.cuh"

namespace lfml {

typedef uint32_t u32;
typedef uint64_t u64;

// ---- the field policies ----------------------------------------------------------------------------------------------------------------------------------
template <bool NU>
struct GoldMls {
    typedef u64 W;
    typedef u64 Part;
    typedef lf::DevCrt Tab;
    typedef lf::Fq3 Ext;
    static constexpr int TAU = 3, PTS = PTS_GOLD;
    // entries 2b, 2b + 1 of the slot's TAU planes (p = plane 0 of the slot): one 16-byte load per plane (ld is even)
    static __device__ __forceinline__ void load2(const u64 *p, size_t ld, size_t b, Ext &v0, Ext &v1) {
#pragma unroll
        for (int c = 0; c < TAU; c++) {
            const ulonglong2 a = *(const ulonglong2 *)(p + (size_t)c * ld + 2 * b);
            v0.c[c] = a.x; v1.c[c] = a.y;
        }
    }
    static __device__ __forceinline__ Ext zero() { return lf::fq3_zero(); }
    static __device__ __forceinline__ Ext add(Ext a, Ext b) { return lf::fq3_add(a, b); }
    static __device__ __forceinline__ Ext sub(Ext a, Ext b) { return lf::fq3_sub(a, b); }
    static __device__ __forceinline__ Ext mul(Ext a, Ext b, const Tab &t) { return lf::fq3_mul<NU>(a, b, t.nu); }
    static __device__ __forceinline__ Part part(u64 w) { return w; }
    static __device__ __forceinline__ Part part_add(Part a, Part b) { return lf::fq_add(a, b); }
    static __device__ __forceinline__ u64 canon(Part a) { return lf::fq_canon(a); }
    static __device__ __forceinline__ u64 fin_add(u64 a, u64 b) { return lf::fq_add(a, b); }
    static __device__ __forceinline__ u64 fin_done(u64 a) { return a; }
};
struct BbMls {
    typedef lfbb::fe W;
    typedef int64_t Part;
    typedef lfbb::DevBb Tab;
    typedef lfbb::E9 Ext;
    static constexpr int TAU = lfbb::TAU, PTS = PTS_BB;
    static __device__ __forceinline__ void load2(const W *p, size_t ld, size_t b, Ext &v0, Ext &v1) {
#pragma unroll
        for (int c = 0; c < TAU; c++) {
            const int2 a = *reinterpret_cast<const int2 *>(p + (size_t)c * ld + 2 * b);
            v0.c[c] = a.x; v1.c[c] = a.y;
        }
    }
    static __device__ __forceinline__ Ext zero() { return lfbb::e9_zero(); }
    static __device__ __forceinline__ Ext add(const Ext &a, const Ext &b) { return lfbb::e9_add(a, b); }
    static __device__ __forceinline__ Ext sub(const Ext &a, const Ext &b) { return lfbb::e9_sub(a, b); }
    static __device__ __forceinline__ Ext mul(const Ext &a, const Ext &b, const Tab &t) { return lfbb::e9_mul(a, b, t.nu); }
    // block partials are plain signed sums of centred words (|w| <= H < 2^30: 2^8 wave and block terms, then MAX_BLOCKS rows reduced mod p one by one)
    static __device__ __forceinline__ Part part(W w) { return (Part)w; }
    static __device__ __forceinline__ Part part_add(Part a, Part b) { return a + b; }
    static __device__ __forceinline__ u64 canon(Part a) { return lfbb::to_canon(lfbb::fred(a)); }
    static __device__ __forceinline__ u64 fin_add(u64 a, u64 b) { return a + b; }
    static __device__ __forceinline__ u64 fin_done(u64 a) { return a % lfbb::BB_P; }
};

// the descriptor in the kernel-argument segment (it is the first argument: offset 0)
static __device__ __forceinline__ const Desc *desc_args() { return (const Desc *)__builtin_amdgcn_kernarg_segment_ptr(); }

// factor k of the descriptor at pair b: its value at the group's first point x0 and its step
template <class P>
static __device__ __forceinline__ void mls_factor(const Desc *d, u32 k, const typename P::W *__restrict__ tab, size_t ld, u32 slot, size_t b, u32 x0,
                                                  typename P::Ext &val, typename P::Ext &st) {
    constexpr int TAU = P::TAU, RE = 8 * TAU;
    typename P::Ext v0, v1;
    P::load2(tab + ((size_t)((d->idx4[k >> 2] >> (8 * (k & 3))) & 0xffu) * RE + (size_t)TAU * slot) * ld, ld, b, v0, v1);
    st = P::sub(v1, v0);
    val = v0;
    for (u32 j = 0; j < x0; j++) val = P::add(val, st);
}

template <class P>
__global__ void __launch_bounds__(256) k_mls_round(Desc, typename P::Tab t, const typename P::W *__restrict__ tab, size_t ld, size_t npairs,
                                                   const typename P::W *__restrict__ coef, typename P::Part *__restrict__ partial) {
    typedef typename P::Ext Ext;
    typedef typename P::Part Part;
    constexpr int TAU = P::TAU, G = P::PTS, RE = 8 * TAU;
    const Desc *d = desc_args();
    const u32 slot = blockIdx.y, x0 = blockIdx.z * G, q = d->q;
    Ext acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = P::zero();
    for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < npairs; b += (size_t)gridDim.x * 256) {
#pragma unroll 1
        for (u32 i = 0; i < q; i++) {
            const u32 cls = (d->cls[i] >> (2 * slot)) & 3u;
            if (cls == COEF_ZERO) continue;   // (wave-uniform: the class is a function of the term and the slot)
            const u32 k0 = d->off[i], k1 = d->off[i + 1];
            Ext pr[G], val, st;
            mls_factor<P>(d, k0, tab, ld, slot, b, x0, val, st);
#pragma unroll
            for (int g = 0; g < G; g++) {
                pr[g] = val;
                if (g + 1 < G) val = P::add(val, st);
            }
#pragma unroll 1
            for (u32 k = k0 + 1; k < k1; k++) {
                mls_factor<P>(d, k, tab, ld, slot, b, x0, val, st);
#pragma unroll
                for (int g = 0; g < G; g++) {
                    pr[g] = P::mul(pr[g], val, t);
                    if (g + 1 < G) val = P::add(val, st);
                }
            }
            if (cls == COEF_GENERAL) {
                Ext cf;
                const typename P::W *cw = coef + ((size_t)i * 8 + slot) * TAU;
#pragma unroll
                for (int c = 0; c < TAU; c++) cf.c[c] = cw[c];
#pragma unroll
                for (int g = 0; g < G; g++) pr[g] = P::mul(pr[g], cf, t);
            }
            if (cls == COEF_MINUS_ONE) {
#pragma unroll
                for (int g = 0; g < G; g++) acc[g] = P::sub(acc[g], pr[g]);
            } else {
#pragma unroll
                for (int g = 0; g < G; g++) acc[g] = P::add(acc[g], pr[g]);
            }
        }
    }
    // pairs of the block -> one partial row: wave64 shuffle reduction, then the four wave sums through LDS
    __shared__ Part sm[4][G * TAU];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int c = 0; c < TAU; c++) {
            Part v = P::part(acc[g].c[c]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v = P::part_add(v, (Part)__shfl_down((unsigned long long)v, o, 64));
            if (lane == 0) sm[wave][g * TAU + c] = v;
        }
    __syncthreads();
    if (threadIdx.x < G * TAU) {
        const u32 g = threadIdx.x / TAU, c = threadIdx.x % TAU;
        const size_t row = (size_t)gridDim.z * G * RE;   // words of a block's row: [point][slot][TAU]
        partial[(size_t)blockIdx.x * row + ((size_t)(x0 + g) * 8 + slot) * TAU + c] =
            P::part_add(P::part_add(sm[0][threadIdx.x], sm[1][threadIdx.x]), P::part_add(sm[2][threadIdx.x], sm[3][threadIdx.x]));
    }
}

// out[w] = canonical(sum_b partial[b * row + w]), w < npts * RE (the points past the degree of the last group stay in the partial rows): one wave per word,
// lane l takes rows l, l + 64, ..., then the wave64 shuffle reduction (the k_reduce_rows pattern).  Every row word is made canonical before it is added: the
// sum is P::fin_add of canonical words (field additions on Goldilocks; plain additions of at most MAX_BLOCKS words below 2^31 on BabyBear, reduced once)
template <class P>
__global__ void __launch_bounds__(64) k_mls_finish(const typename P::Part *__restrict__ partial, u32 nblocks, u32 row, u64 *__restrict__ out) {
    const u32 w = blockIdx.x;
    u64 s = 0;
    for (u32 b = threadIdx.x; b < nblocks; b += 64) s = P::fin_add(s, P::canon(partial[(size_t)b * row + w]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = P::fin_add(s, (u64)__shfl_down((unsigned long long)s, o, 64));
    if (threadIdx.x == 0) out[w] = P::fin_done(s);
}

template <class P>
static int launch(const typename P::Tab &t, const Desc &d, const typename P::W *tab, size_t ld, size_t npairs, const typename P::W *coef,
                  typename P::Part *partial, u64 *out, hipStream_t s) {
    constexpr u32 G = P::PTS, RE = 8 * P::TAU;
    if (!npairs || !d.npts || d.npts > MAX_DEGREE + 1 || !d.q || d.q > MAX_TERMS) return -1;
    const u32 gb = round_blocks(npairs), gz = point_groups(d.npts, G), row = gz * G * RE, nwords = d.npts * RE;
    hipLaunchKernelGGL(k_mls_round<P>, dim3(gb, 8, gz), dim3(256), 0, s, d, t, tab, ld, npairs, coef, partial);
    hipLaunchKernelGGL(k_mls_finish<P>, dim3(nwords), dim3(64), 0, s, partial, gb, row, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_mls_round(const lf::DevCrt &t, const Desc &d, const uint64_t *tab, size_t ld, size_t npairs, const uint64_t *coef, uint64_t *partial, uint64_t *out,
                     hipStream_t s) {
    return t.nu2p40 ? launch<GoldMls<true>>(t, d, tab, ld, npairs, coef, partial, out, s) : launch<GoldMls<false>>(t, d, tab, ld, npairs, coef, partial, out, s);
}
int launch_mls_round(const lfbb::DevBb &t, const Desc &d, const int32_t *tab, size_t ld, size_t npairs, const int32_t *coef, int64_t *partial, uint64_t *out,
                     hipStream_t s) {
    return launch<BbMls>(t, d, tab, ld, npairs, coef, partial, out, s);
}

}  // namespace lfml
