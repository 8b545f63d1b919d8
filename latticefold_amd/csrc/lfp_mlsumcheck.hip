// lfp_mlsumcheck.hip -- MLSumcheck::prove_as_subprotocol (latticefold utils/sumcheck/prover.rs:111-143) over ANY sum of products of MLE tables on the Frog
// ring Z_p[X]/(X^16 + 1), coefficient form: the round kernel of lfplus_mlsumcheck_* (include/lfplus.h; host driver lfp_mlsumcheck.cpp).  The three protocol
// sumchecks of the slice keep their own kernels (lfp_rgchk.hip): this one INTERPRETS a product list and pays for it -- (|S_i| - 1) negacyclic products per term
// and point where k_r1cs_round gets by with three per pair.
#include "lfp_field.cuh"
namespace lfp {
// one coefficient of a negacyclic product: aM the 16 Montgomery words of the left operand, b the 16 canonical words of the right one.  One lazy signed 160-bit sum
// and one reduction (as r1cs_negacyclic); the bias covers the 16 subtracted products of THIS sum only, so nothing else is ever added to the accumulator
__device__ __forceinline__ u64 mls_negacyclic(const u64 *aM, const u64 *b, u32 c) {
    Acc160 n;
    acc160_bias16(n);
#pragma unroll
    for (u32 j = 0; j < 16; j++) acc160_mad_signed(n, aM[j], b[(c - j) & 15], j > c);
    return acc160_red(n);
}
// thread = (pair pl, coefficient c), 16 pairs per workgroup and pass.  Dynamic LDS, u64 words:
//   acc[degree + 1][256]   the thread's own running sums per point (a register array indexed by the point would go to scratch)
//   val[nt][256]           every table's value at the current point: the operands of the products, read by the 16 lanes of the pair
//   pr[2][256]             the running product of a chain in Montgomery form, double-buffered: ONE barrier per product
//   cf[nterms][16]         the coefficients
// The steps (hi - lo) stay in registers, selected by fully unrolled loops guarded with t < nt (constant indices: lf_lin_wide.hip tells what a run-time index costs).
// Every barrier below sits in control flow that depends on the descriptor and on blockIdx alone: all 256 threads reach it, also in a pass whose 16-pair group is
// partly or wholly out of range -- those lanes carry zero values and zero steps and add zeros.
template <bool FUSED>
__global__ void __launch_bounds__(256) k_mls_round(const u64 *__restrict__ in, size_t ld_in, size_t half, MlsDesc d, const u64 *__restrict__ coef, u64 rM, u64 *__restrict__ out,
                                                   size_t ld_out, u64 *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) u64 mls_lds[];      // (no static LDS in this kernel: the dynamic region starts at 0; every carve is a multiple of 128 bytes)
    const u32 tid = threadIdx.x, c = tid & 15, pl = tid >> 4, np = d.degree + 1;
    u64 *acc = mls_lds, *val = acc + np * 256, *pr = val + d.nt * 256, *cf = pr + 512;
    for (u32 x = 0; x < np; x++) acc[x * 256 + tid] = 0;
    for (u32 i = tid; i < d.nterms * 16; i += 256) cf[i] = coef[i];      // (visible behind the first barrier of the first pass; every workgroup has one)
    auto fixw = [&](u64 lo, u64 hi) { return add_p(lo, mont_mul(rM, sub_p(hi, lo))); };
    u32 buf = 0;
    for (size_t base = (size_t)blockIdx.x * 16; base < half; base += (size_t)gridDim.x * 16) {
        const size_t b = base + pl;
        u64 st[16];
#pragma unroll
        for (u32 t = 0; t < 16; t++) {
            st[t] = 0;
            if (t < d.nt) {
                u64 v0 = 0, v1 = 0;
                if (b < half) {
                    if (FUSED) {
                        const u64 *gp = in + ((size_t)t * ld_in + 4 * b) * 16 + c;
                        v0 = fixw(gp[0], gp[16]); v1 = fixw(gp[32], gp[48]);
                        u64 *op = out + ((size_t)t * ld_out + 2 * b) * 16 + c;
                        op[0] = v0; op[16] = v1;
                    } else {
                        const u64 *gp = in + ((size_t)t * ld_in + 2 * b) * 16 + c;
                        v0 = gp[0]; v1 = gp[16];
                    }
                }
                val[t * 256 + tid] = v0;
                st[t] = sub_p(v1, v0);
            }
        }
        for (u32 x = 0; x < np; x++) {
            if (x) {      // the next point by one addition of the step (prover.rs:128-134); the barrier that ended the previous point lets the owner write
#pragma unroll
                for (u32 t = 0; t < 16; t++)
                    if (t < d.nt) val[t * 256 + tid] = add_p(val[t * 256 + tid], st[t]);
            }
            __syncthreads();
            u64 tot = 0;
            for (u32 i = 0; i < d.nterms; i++) {
                const u32 cls = d.cls[i];
                if (cls == MLS_ZERO) continue;
                u64 cur = val[(u32)d.idx[d.off[i]] * 256 + tid];
                for (u32 k = (u32)d.off[i] + 1; k < d.off[i + 1]; k++) {      // the chain: each product is a canonical word before the next
                    pr[buf * 256 + tid] = to_mont(cur);
                    __syncthreads();
                    cur = mls_negacyclic(pr + buf * 256 + pl * 16, val + (u32)d.idx[k] * 256 + pl * 16, c);
                    buf ^= 1;
                }
                if (cls == MLS_GENERAL) {
                    pr[buf * 256 + tid] = to_mont(cur);
                    __syncthreads();
                    cur = mls_negacyclic(pr + buf * 256 + pl * 16, cf + i * 16, c);
                    buf ^= 1;
                }
                tot = cls == MLS_MINUS_ONE ? sub_p(tot, cur) : add_p(tot, cur);
            }
            acc[x * 256 + tid] = add_p(acc[x * 256 + tid], tot);
            __syncthreads();      // (the pair's lanes have read val: its owner may move on)
        }
    }
    __syncthreads();
    if (tid < np * 16) {          // (degree + 1) * 16 <= 144 outputs: the sum over the 16 pairs
        const u32 x = tid >> 4;
        u64 t = 0;
        for (u32 p = 0; p < 16; p++) t = add_p(t, acc[x * 256 + p * 16 + c]);
        part[(size_t)blockIdx.x * np * 16 + tid] = t;
    }
}
__global__ void __launch_bounds__(256) k_mls_final(const u64 *__restrict__ in, size_t ld_in, u32 nt, u64 rM, u64 *__restrict__ out) {
    const u32 t = threadIdx.x >> 4, c = threadIdx.x & 15;
    if (t >= nt) return;
    const u64 *gp = in + (size_t)t * ld_in * 16 + c;
    const u64 lo = gp[0], hi = gp[16];
    out[t * 16 + c] = add_p(lo, mont_mul(rM, sub_p(hi, lo)));
}
static size_t mls_lds_bytes(const MlsDesc &d) { return ((size_t)(d.degree + 1 + d.nt + 2) * 256 + (size_t)d.nterms * 16) * 8; }      // <= 56 KB at the full envelope
u32 mls_round_blocks(size_t half, u32 cap) {
    const size_t b = (half + 15) / 16;
    return (u32)(b < 1 ? 1 : (b > cap ? cap : b));
}
void launch_mls_round(const u64 *in, size_t ld_in, size_t half, const MlsDesc &d, const u64 *coef, u32 blocks, u64 *part, hipStream_t s) {
    hipLaunchKernelGGL((k_mls_round<false>), dim3(blocks), dim3(256), mls_lds_bytes(d), s, in, ld_in, half, d, coef, (u64)0, (u64 *)nullptr, (size_t)0, part);
}
void launch_mls_round_fused(const u64 *in, size_t ld_in, size_t half, const MlsDesc &d, const u64 *coef, u64 rM, u64 *out, size_t ld_out, u32 blocks, u64 *part, hipStream_t s) {
    hipLaunchKernelGGL((k_mls_round<true>), dim3(blocks), dim3(256), mls_lds_bytes(d), s, in, ld_in, half, d, coef, rM, out, ld_out, part);
}
void launch_mls_final(const u64 *in, size_t ld_in, u32 nt, u64 rM, u64 *out, hipStream_t s) {
    hipLaunchKernelGGL(k_mls_final, dim3(1), dim3(256), 0, s, in, ld_in, nt, rM, out);
}
}  // namespace lfp
