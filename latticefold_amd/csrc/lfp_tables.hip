// lfp_tables.hip -- MLE tables on arrays (lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t and their _device forms,
// include/lfplus.h; host bodies lfp_tables.cpp): the eq(r, .) table, evaluations and partial evaluations of tables of GENERAL ring elements of
// Z_p[X]/(X^16 + 1) at a point of F_p words, and M_j^T v on the resident matrices.  Coefficient form, 16 canonical words per element, AoS.
//   Exactness.  Every result is a canonical word of an exact sum mod p, so it does not depend on the order or the grouping of the terms: fixing nfix
// variables one at a time (lo + r (hi - lo)) and the one weighted sum sum_t eq(r, t) T[y 2^nfix + t] give the same words; so do the columns of M^T v whatever
// the order of their entries and whichever path sums them.
//   Memory.  An element is 128 bytes: 8 lanes fetch it as 8 consecutive 16-byte pairs, so every request is a whole element and a wave covers 8 elements (1 KB)
// per load.  eval and fix read every table once; the words of a pair are tested against p where they are loaded.
//   eq weights.  Never a ring table.  eq(r, x) = L[x mod 2^lo] * H(x >> lo): L, the weights of the low lo = min(nv, 10) variables, is built by each workgroup
// in LDS (8 KB); H, the product over the high variables, is one value per chunk of 2^lo entries and is computed when a workgroup takes the chunk (nv - lo
// products for 2^lo / 32 passes).  Weights are Montgomery words, table words canonical: a lazy 160-bit sum of their products reduces to the canonical sum.
//   Arithmetic.  Unsigned lazy sums (acc160_mad) for eval and fix.  spmv_t multiplies two CANONICAL operands (the resident transposed values and v): the
// signed lazy sum of a column reduces to sum * 2^-64, one more Montgomery product with 2^128 gives the sum.  The bias of that accumulator covers 1024
// subtracted products = 64 negacyclic products (SPT_FLUSH); a 16-lane group reduces and restarts it every 64 entries.
#include "lfp_field.cuh"
namespace lfp {
// prod_{i < nbits} (bit i of x ? r_(first + i) : 1 - r_(first + i)), Montgomery; the empty product is 1
__device__ __forceinline__ u64 tab_eq_bits(const TabPoint &pt, u32 first, u32 nbits, u64 x) {
    u64 w = pt.oneM;
    for (u32 i = 0; i < nbits; i++) {
        const u64 r = pt.rM[first + i];
        w = mont_mul(w, ((x >> i) & 1) ? r : sub_p(pt.oneM, r));
    }
    return w;
}

// ---- eq(point, .) as constant polynomials: a workgroup takes chunks of 256 entries; thread t computes entry t of the chunk, the stores leave as 16-byte pairs
__global__ void __launch_bounds__(256) k_tab_eq(TabPoint pt, u32 nv, u64 *__restrict__ out) {
    __shared__ u64 sv[256];
    const u32 tid = threadIdx.x, lo = nv < 8 ? nv : 8, q = tid & 7;
    const u64 len = 1ull << nv, chunks = (len + 255) >> 8;
    const u64 wl = tab_eq_bits(pt, 0, lo, tid);                                      // (used by the threads below 2^lo only)
    for (u64 ch = blockIdx.x; ch < chunks; ch += gridDim.x) {                        // (the trip count depends on blockIdx alone: every thread reaches the barriers)
        sv[tid] = mont_mul(wl, from_mont(tab_eq_bits(pt, lo, nv - lo, ch)));         // Montgomery x canonical: the canonical product
        __syncthreads();
#pragma unroll
        for (u32 k = 0; k < 8; k++) {
            const u32 e = k * 32 + (tid >> 3);
            const u64 x = (ch << 8) + e;
            if (x < len) *(ulonglong2 *)(out + x * 16 + 2 * q) = make_ulonglong2(q ? 0 : sv[e], 0);
        }
        __syncthreads();
    }
}
void launch_tab_eq(const TabPoint &pt, u32 nv, u64 *out, u32 cap, hipStream_t s) {
    const u64 chunks = ((1ull << nv) + 255) >> 8;
    hipLaunchKernelGGL(k_tab_eq, dim3((u32)(chunks < cap ? chunks : cap)), dim3(256), 0, s, pt, nv, out);
}

// ---- out[j] = sum_{x < len} eq(point, x) T_j[x]: grid (blocks, ntables); lane = (entry el of a pass of 32, pair q); the workgroups of a table stride over its chunks
__global__ void __launch_bounds__(256) k_tab_eval(const u64 *__restrict__ tables, u64 len, TabPoint pt, u32 nv, u64 *__restrict__ part, u32 *flag) {
    __shared__ u64 sL[1u << TAB_LO];
    __shared__ u64 sred[4][16];
    const u32 tid = threadIdx.x, q = tid & 7, el = tid >> 3, lo = nv < TAB_LO ? nv : TAB_LO;
    const u32 chunk = 1u << lo;
    const u64 chunks = (len + chunk - 1) >> lo;
    for (u32 i = tid; i < chunk; i += 256) sL[i] = tab_eq_bits(pt, 0, lo, i);
    __syncthreads();
    const u64 *T = tables + (u64)blockIdx.y * len * 16;
    Acc160 a0, a1;
    acc160_zero(a0);
    acc160_zero(a1);
    bool bad = false;
    for (u64 ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const u64 wh = tab_eq_bits(pt, lo, nv - lo, ch);
        for (u32 e0 = el; e0 < chunk; e0 += 128) {                                   // four passes of 32 entries: their loads are issued before the first product
            ulonglong2 v[4];
#pragma unroll
            for (u32 k = 0; k < 4; k++) {
                const u32 e = e0 + 32 * k;
                const u64 x = (ch << lo) + e;
                v[k] = make_ulonglong2(0, 0);                                        // (entries from len on count as zero)
                if (e < chunk && x < len) v[k] = *(const ulonglong2 *)(T + x * 16 + 2 * q);
            }
#pragma unroll
            for (u32 k = 0; k < 4; k++) {
                const u32 e = e0 + 32 * k;
                bad |= v[k].x >= P || v[k].y >= P;
                if (e < chunk) {
                    const u64 w = mont_mul(sL[e], wh);
                    acc160_mad(a0, w, v[k].x);
                    acc160_mad(a1, w, v[k].y);
                }
            }
        }
    }
    // the 8 entries of a wave's pass, pair by pair, across the wave; the four waves through LDS
    u64 r0 = acc160_red(a0), r1 = acc160_red(a1);
#pragma unroll
    for (u32 m = 8; m < 64; m <<= 1) {
        r0 = add_p(r0, __shfl_xor(r0, m));
        r1 = add_p(r1, __shfl_xor(r1, m));
    }
    if ((tid & 63) < 8) { sred[tid >> 6][2 * q] = r0; sred[tid >> 6][2 * q + 1] = r1; }
    __syncthreads();
    if (tid < 16) part[((u64)blockIdx.y * gridDim.x + blockIdx.x) * 16 + tid] = add_p(add_p(sred[0][tid], sred[1][tid]), add_p(sred[2][tid], sred[3][tid]));
    if (__any(bad) && (tid & 63) == 0) atomicOr(flag, 1u);
}
// one workgroup per table: 16 lanes read the 16 words of a block's share, the 16 lane groups stride over the blocks and meet as the waves of k_tab_eval do
__global__ void __launch_bounds__(256) k_tab_eval_sum(const u64 *__restrict__ part, u32 blocks, u64 *__restrict__ out) {
    __shared__ u64 sred[4][16];
    const u32 tid = threadIdx.x, w = tid & 15;
    const u64 *p = part + (u64)blockIdx.x * blocks * 16 + w;
    u64 s = 0;
#pragma unroll 4
    for (u32 b = tid >> 4; b < blocks; b += 16) s = add_p(s, p[(u64)b * 16]);
    s = add_p(s, __shfl_xor(s, 16));
    s = add_p(s, __shfl_xor(s, 32));
    if ((tid & 63) < 16) sred[tid >> 6][w] = s;
    __syncthreads();
    if (tid < 16) out[blockIdx.x * 16 + tid] = add_p(add_p(sred[0][tid], sred[1][tid]), add_p(sred[2][tid], sred[3][tid]));
}
u32 tab_eval_blocks(u64 len, u32 nv, u32 ntables, u32 cap) {
    const u32 lo = nv < TAB_LO ? nv : TAB_LO;
    const u64 chunks = (len + (1ull << lo) - 1) >> lo;
    const u32 per = cap / ntables ? cap / ntables : 1;
    return (u32)(chunks < per ? chunks : per);
}
void launch_tab_eval(const u64 *tables, u32 ntables, u64 len, const TabPoint &pt, u32 nv, u32 blocks, u64 *part, u64 *out, u32 *flag, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_eval, dim3(blocks, ntables), dim3(256), 0, s, tables, len, pt, nv, part, flag);
    hipLaunchKernelGGL(k_tab_eval_sum, dim3(ntables), dim3(256), 0, s, (const u64 *)part, blocks, out);
}

// ---- fix_variables of the lowest nf <= TAB_FIX variables: thread = (output entry y, pair q), one weighted sum over the 2^nf entries below y
__global__ void __launch_bounds__(256) k_tab_fix(const u64 *__restrict__ in, u64 ld_in, u64 nout, TabPoint pt, u32 nf, u64 *__restrict__ out, u32 *flag) {
    __shared__ u64 sw[1u << TAB_FIX];
    const u32 tid = threadIdx.x, S = 1u << nf;
    if (tid < S) sw[tid] = tab_eq_bits(pt, 0, nf, tid);
    __syncthreads();
    const u64 id = (u64)blockIdx.x * 256 + tid, y = id >> 3;
    const u32 q = (u32)id & 7;
    bool bad = false;
    if (y < nout) {
        const u64 *T = in + ((u64)blockIdx.y * ld_in + (y << nf)) * 16 + 2 * q;
        Acc160 a0, a1;
        acc160_zero(a0);
        acc160_zero(a1);
        for (u32 t = 0; t < S; t++) {
            const ulonglong2 v = *(const ulonglong2 *)(T + (u64)t * 16);
            bad |= v.x >= P || v.y >= P;
            acc160_mad(a0, sw[t], v.x);
            acc160_mad(a1, sw[t], v.y);
        }
        *(ulonglong2 *)(out + ((u64)blockIdx.y * nout + y) * 16 + 2 * q) = make_ulonglong2(acc160_red(a0), acc160_red(a1));
    }
    if (__any(bad) && (tid & 63) == 0) atomicOr(flag, 1u);
}
void launch_tab_fix(const u64 *in, u64 ld_in, u32 ntables, u64 nout, const TabPoint &pt, u32 nf, u64 *out, u32 *flag, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_fix, dim3((u32)((nout * 8 + 255) / 256), ntables), dim3(256), 0, s, in, ld_in, nout, pt, nf, out, flag);
}

// ---- out = M^T v on the transposed structure the resident matrix carries (colptr, rowidx, canonical values in column order)
// 960 subtracted products of 64 negacyclic products cannot exhaust 1024 p 2^64; with all 1024 added the integer stays below 2^139 (as lfp_ring_ops.hip's bias)
__device__ __forceinline__ void spt_bias(Acc160 &n) { n.a[0] = n.a[1] = 0; n.a[2] = (u32)(P << 10); n.a[3] = (u32)((P << 10) >> 32); n.a[4] = (u32)(P >> 54); }
// n += coefficient c of m * v: the lanes of a 16-lane group hold word c of both operands and fetch the others across the group
__device__ __forceinline__ void spt_mac(Acc160 &n, u64 mc, u64 vc, u32 c) {
#pragma unroll
    for (u32 j = 0; j < 16; j++) acc160_mad_signed(n, __shfl(mc, (int)j, 16), __shfl(vc, (int)((c - j) & 15), 16), j > c);
}
// the canonical value of the lazy sum; the accumulator restarts
__device__ __forceinline__ u64 spt_flush(Acc160 &n) {
    const u64 r = mont_mul(acc160_red(n), R2);
    spt_bias(n);
    return r;
}
// A workgroup takes 16 columns.  A column of at most SPT_HEAVY entries belongs to one 16-lane group (lane = coefficient).  The others are taken one after the
// other by all 16 groups, group g the entries g, g + 16, ..: the four groups of a wave meet across the wave, the four waves in LDS.  Every barrier sits in
// control flow that depends on colptr alone.
__global__ void __launch_bounds__(256) k_spmv_t(const u32 *__restrict__ colptr, const u32 *__restrict__ rowidx, const u64 *__restrict__ val, const u64 *__restrict__ v,
                                                u64 n, u64 *__restrict__ out) {
    __shared__ u32 slo[16], scnt[16];
    __shared__ u64 sred[4][16];
    const u32 tid = threadIdx.x, c = tid & 15, grp = tid >> 4;
    const u64 col = (u64)blockIdx.x * 16 + grp;
    u32 lo = 0, cnt = 0;
    if (col < n) { lo = colptr[col]; cnt = colptr[col + 1] - lo; }
    if (c == 0) { slo[grp] = lo; scnt[grp] = cnt; }
    Acc160 a;
    spt_bias(a);
    if (col < n && cnt <= SPT_HEAVY) {
        for (u32 k = lo; k < lo + cnt; k++) spt_mac(a, val[(u64)k * 16 + c], v[(u64)rowidx[k] * 16 + c], c);
        out[col * 16 + c] = spt_flush(a);
    }
    __syncthreads();
    for (u32 g = 0; g < 16; g++) {
        const u32 hc = scnt[g], hlo = slo[g];
        if (hc <= SPT_HEAVY) continue;
        u64 s = 0;
        u32 pending = 0;
        for (u32 k = grp; k < hc; k += 16) {
            spt_mac(a, val[(u64)(hlo + k) * 16 + c], v[(u64)rowidx[hlo + k] * 16 + c], c);
            if (++pending == SPT_FLUSH) { s = add_p(s, spt_flush(a)); pending = 0; }
        }
        s = add_p(s, spt_flush(a));
        s = add_p(s, __shfl_xor(s, 16));
        s = add_p(s, __shfl_xor(s, 32));
        if ((tid & 63) < 16) sred[tid >> 6][c] = s;
        __syncthreads();
        if (tid < 16) out[((u64)blockIdx.x * 16 + g) * 16 + tid] = add_p(add_p(sred[0][tid], sred[1][tid]), add_p(sred[2][tid], sred[3][tid]));
        __syncthreads();
    }
}
void launch_spmv_t(const u32 *colptr, const u32 *rowidx, const u64 *val, const u64 *v, u64 n, u64 *out, hipStream_t s) {
    hipLaunchKernelGGL(k_spmv_t, dim3((u32)((n + 15) / 16)), dim3(256), 0, s, colptr, rowidx, val, v, n, out);
}
}  // namespace lfp
