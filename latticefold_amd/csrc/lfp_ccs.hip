// lfp_ccs.hip -- the round kernel of lfplus_ccs_linearize (include/lfplus.h; host driver lfp_protocol.cpp): one round of the degree-(d + 1) sumcheck of
//      eq(r, x) * sum_{i < q} c_i prod_{j in S_i} g_j(x),      g_j = M_j f,
// on the Frog ring Z_p[X]/(X^16 + 1), coefficient form -- ComR1CS::linearize (r1cs.rs:76-139) with the comb function of a CCS shape in place of ga gb - gc.
//   Cost.  Per pair and point: sum_i (|S_i| - 1) negacyclic products, plus one per GENERAL coefficient c_i; none for eq, none for a coefficient 0, +1, -1 or a
// base-field constant.  eq is the one-word-per-row table E: it is stepped along X like the tables and multiplies the FINISHED sum of the point word by word
// (one mont_mul per coefficient).  k_mls_round on [eq, g_0 ..] spends sum_i |S_i| products (eq is a factor of every term) and reads 16 words of eq per row.
//   Barriers.  Per point: one that publishes the tables' values, then one per product LEVEL -- level l forms product l of EVERY chain between one pair of
// barriers -- so 1 + (maxlev - 1) with maxlev = max_i (|S_i| + [c_i general]) <= d + 1, whatever q is.  The values and the running products are double-buffered
// in LDS, which is what lets one barrier separate a level's reads from the next writes of the same buffer.
//   Every barrier sits in control flow that depends on the descriptor and on blockIdx alone (see lfp_mlsumcheck.hip): all 256 threads reach it, also in a pass
// whose 16-pair group is partly or wholly out of range -- those lanes carry zero values, zero steps and a zero eq word, and add zeros.
//   LDS layout (dynamic; a general coefficient is read from global memory, 16 words that every lane shares).  val[2][t][256] and pr[2][nslots][256] u64: lane
// (pair pl, coefficient c) owns word pl * 16 + c of a row.  A product reads pr[.][pl * 16 + j] (one address per pair: a broadcast) and
// val[.][pl * 16 + ((c - j) & 15)] (the pair's 16 words, rotated): the two pairs of a 32-lane ds_read_b64 group cover one whole 256-byte bank row, each bank
// once -- conflict-free without padding.
#include "lfp_field.cuh"
namespace lfp {
// one coefficient of a negacyclic product: aM the 16 Montgomery words of the left operand, b the 16 canonical words of the right one; one lazy signed 160-bit sum
// and one reduction (as r1cs_negacyclic / mls_negacyclic)
__device__ __forceinline__ u64 ccs_negacyclic(const u64 *aM, const u64 *b, u32 c) {
    Acc160 n;
    acc160_bias16(n);
#pragma unroll
    for (u32 j = 0; j < 16; j++) acc160_mad_signed(n, aM[j], b[(c - j) & 15], j > c);
    return acc160_red(n);
}
// tot +- c_i * v for a coefficient that needs no product of its own (a general one went through the chain's last level)
__device__ __forceinline__ u64 ccs_add_term(u64 tot, u64 v, u32 cls, u64 cstM) {
    if (cls == CCS_MINUS_ONE) return sub_p(tot, v);
    if (cls == CCS_CONST) return add_p(tot, mont_mul(cstM, v));
    return add_p(tot, v);
}
// thread = (pair pl, coefficient c), 16 pairs per workgroup and pass; NP = d + 2 evaluation points, their running sums in registers (s[k] is only ever indexed
// by an unrolled constant).  The steps (hi - lo) of the tables stay in registers too, selected by fully unrolled loops guarded with j < d.t.
template <int NP, bool FUSED>
__global__ void __launch_bounds__(256) k_ccs_round(const u64 *__restrict__ E, const u64 *__restrict__ G, size_t ld, size_t half, CcsDesc d, const u64 *__restrict__ coef,
                                                   u64 rM, u64 *__restrict__ Eo, u64 *__restrict__ Go, size_t ld_o, u64 *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) u64 ccs_lds[];
    const u32 tid = threadIdx.x, c = tid & 15, pl = tid >> 4;
    u64 *val = ccs_lds, *pr = val + 2 * d.t * 256;
    auto fixw = [&](u64 lo, u64 hi) { return add_p(lo, mont_mul(rM, sub_p(hi, lo))); };
    u64 s[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) s[k] = 0;
    u32 vb = 0, pb = 0;
    for (size_t base = (size_t)blockIdx.x * 16; base < half; base += (size_t)gridDim.x * 16) {
        const size_t b = base + pl;
        u64 e = 0, de = 0, v[8], st[8];
        if (b < half) {
            if (FUSED) {
                e = fixw(E[4 * b], E[4 * b + 1]);
                const u64 e1 = fixw(E[4 * b + 2], E[4 * b + 3]);
                if (c == 0) { Eo[2 * b] = e; Eo[2 * b + 1] = e1; }
                de = sub_p(e1, e);
            } else {
                e = E[2 * b];
                de = sub_p(E[2 * b + 1], e);
            }
        }
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            v[j] = st[j] = 0;
            if (j < d.t && b < half) {
                u64 v1;
                if (FUSED) {
                    const u64 *gp = G + ((size_t)j * ld + 4 * b) * 16 + c;
                    v[j] = fixw(gp[0], gp[16]); v1 = fixw(gp[32], gp[48]);
                    u64 *op = Go + ((size_t)j * ld_o + 2 * b) * 16 + c;
                    op[0] = v[j]; op[16] = v1;
                } else {
                    const u64 *gp = G + ((size_t)j * ld + 2 * b) * 16 + c;
                    v[j] = gp[0]; v1 = gp[16];
                }
                st[j] = sub_p(v1, v[j]);
            }
        }
#pragma unroll 1
        for (u32 x = 0; x < (u32)NP; x++) {
            if (x) {      // the next point by one addition of the step (prover.rs:128-134), eq included
                e = add_p(e, de);
#pragma unroll
                for (u32 j = 0; j < 8; j++) v[j] = add_p(v[j], st[j]);
            }
            u64 *vcur = val + (size_t)vb * d.t * 256;
#pragma unroll
            for (u32 j = 0; j < 8; j++)
                if (j < d.t) vcur[j * 256 + tid] = v[j];
            __syncthreads();
            u64 tot = 0;
            for (u32 i = 0; i < d.q; i++) {      // level 0: a chain's first operand is the lane's own word
                const u32 lev = d.lev[i];
                if (!lev) continue;
                const u64 w = vcur[(u32)d.op[i][0] * 256 + tid];
                if (lev == 1) tot = ccs_add_term(tot, w, d.cls[i], d.cst[i]);
                else pr[(pb * d.nslots + d.slot[i]) * 256 + tid] = to_mont(w);
            }
            for (u32 l = 1; l < d.maxlev; l++) {      // level l: product l of every chain that has one; a chain's intermediate is a canonical word before it is an operand
                __syncthreads();
                for (u32 i = 0; i < d.q; i++) {
                    const u32 lev = d.lev[i];
                    if (l >= lev) continue;
                    const u64 *lhs = pr + (pb * d.nslots + d.slot[i]) * 256 + pl * 16;      // (the two right-hand sides live in different address spaces: two calls)
                    const u64 w = l < d.len[i] ? ccs_negacyclic(lhs, vcur + (u32)d.op[i][l] * 256 + pl * 16, c) : ccs_negacyclic(lhs, coef + i * 16, c);
                    if (l + 1 == lev) tot = ccs_add_term(tot, w, d.cls[i], d.cst[i]);
                    else pr[((pb ^ 1) * d.nslots + d.slot[i]) * 256 + tid] = to_mont(w);
                }
                pb ^= 1;
            }
            const u64 term = mont_mul(e, tot);      // eq: once per point, word-wise, on the finished sum
#pragma unroll
            for (int k = 0; k < NP; k++)
                if ((u32)k == x) s[k] = add_p(s[k], term);
            vb ^= 1;
        }
    }
    __syncthreads();      // (the last level's reads are done: the front of the LDS becomes the block sum's staging)
#pragma unroll
    for (int k = 0; k < NP; k++) ccs_lds[k * 256 + tid] = s[k];
    __syncthreads();
    if (tid < NP * 16) {
        const u32 x = tid >> 4;
        u64 t = 0;
        for (u32 p = 0; p < 16; p++) t = add_p(t, ccs_lds[x * 256 + p * 16 + c]);
        part[(size_t)blockIdx.x * NP * 16 + tid] = t;
    }
}
static size_t ccs_lds_bytes(const CcsDesc &d, u32 np) {      // <= 2 * (8 + 8) * 2 KB = 64 KB at the full envelope; the R1CS shape takes 16 KB
    const size_t carve = (size_t)2 * (d.t + d.nslots) * 256 * 8, stage = (size_t)np * 256 * 8;
    return carve > stage ? carve : stage;
}
u32 ccs_round_blocks(size_t half, u32 cap) {
    const size_t b = (half + 15) / 16;
    return (u32)(b < 1 ? 1 : (b > cap ? cap : b));
}
template <bool FUSED>
static void ccs_launch(u32 np, u32 blocks, size_t lds, hipStream_t s, const u64 *E, const u64 *G, size_t ld, size_t half, const CcsDesc &d, const u64 *coef, u64 rM, u64 *Eo,
                       u64 *Go, size_t ld_o, u64 *part) {
#define CCS_CASE(N) case N: hipLaunchKernelGGL((k_ccs_round<N, FUSED>), dim3(blocks), dim3(256), lds, s, E, G, ld, half, d, coef, rM, Eo, Go, ld_o, part); break;
    switch (np) {
        CCS_CASE(3) CCS_CASE(4) CCS_CASE(5) CCS_CASE(6) CCS_CASE(7) CCS_CASE(8) CCS_CASE(9)
        default: break;      // (the host validates 1 <= d <= 7 before anything is launched)
    }
#undef CCS_CASE
}
void launch_ccs_round(const u64 *E, const u64 *G, size_t ld, size_t half, const CcsDesc &d, u32 np, const u64 *coef, u32 blocks, u64 *part, hipStream_t s) {
    ccs_launch<false>(np, blocks, ccs_lds_bytes(d, np), s, E, G, ld, half, d, coef, (u64)0, (u64 *)nullptr, (u64 *)nullptr, (size_t)0, part);
}
void launch_ccs_round_fused(const u64 *E, const u64 *G, size_t ld, size_t half, const CcsDesc &d, u32 np, const u64 *coef, u64 rM, u64 *Eo, u64 *Go, size_t ld_o, u32 blocks,
                            u64 *part, hipStream_t s) {
    ccs_launch<true>(np, blocks, ccs_lds_bytes(d, np), s, E, G, ld, half, d, coef, rM, Eo, Go, ld_o, part);
}
}  // namespace lfp
