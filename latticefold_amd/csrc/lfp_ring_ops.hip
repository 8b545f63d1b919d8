// lfp_ring_ops.hip -- ring arithmetic on arrays (lfplus_ring_mul / lfplus_ring_mul_device, include/lfplus.h; host bodies lfp_ring_ops.cpp): sums of negacyclic
// products in Z_p[X]/(X^16 + 1), coefficient form, over arrays of ring elements.
//   mode 0 (element-wise): out[x] = sum_{i < n_terms} a_i[x] * b_i[x]          mode 1 (broadcast): out[x] = sum_i a_i[x] * b_i
// Mapping: the slice's -- thread = (element pl, coefficient c), 16 lanes per element, 16 elements per 256-thread workgroup and pass; the workgroups stride over
// the 16-element groups with a capped grid.
//   Memory.  A group of one table is 2 KB: 128 lanes fetch it as 128 consecutive 16-byte pairs (whole 128-byte elements, coalesced).  The two halves of the
// workgroup fetch the two operand groups of a step: a_i and b_i in mode 0, a_i and a_(i+1) in mode 1 (b is resident in LDS there; only a streams).  The words of a
// pair are tested against p where they are loaded.  Results leave as 16-byte pairs too: the even coefficient lane takes its neighbour's word across lanes.
//   Operand exchange: through LDS, not across lanes.  A lane needs all 16 words of one operand and a rotation of all 16 of the other, and the words arrive in
// another layout (lane = pair of a 2 KB group) than they are used in (lane = coefficient): the transposition needs LDS anyway, the 16 words of the Montgomery
// operand then come as broadcast reads and the rotated ones as one conflict-free 8-byte read each (two elements = 256 bytes = the 64 banks of a 32-lane group);
// rotating both operands through DPP rows instead would cost 2 x 15 two-register moves per product on the VALU, which is the unit this kernel is short of.
//   Arithmetic.  One operand in Montgomery form (mode 0: a, converted by the lanes that load it; mode 1: b, converted once on the host), the other canonical;
// ONE lazy signed 160-bit sum per output coefficient over all n_terms products and ONE reduction.
//   The double buffer.  A step writes its operands to one half of `sbuf`, passes ONE barrier and reads them; the next step writes the other half.  A half is
// written again two steps later, behind the barrier of the step in between, which no thread passes before it has finished reading.  The next step's global loads
// are issued before the barrier and land while the products run.
//   In place (out == a, or out == b in mode 0, with n_terms == 1).  Every word of both operands of a group is loaded before the barrier of the group's last step;
// its results are stored after that barrier, and no other workgroup touches the group.  The loads issued ahead belong to the NEXT group of this workgroup.
// Every barrier sits in control flow that depends on blockIdx, count and n_terms alone: all 256 threads reach it, also in a group that is partly out of range
// (those lanes carry zeros and store nothing).
#include "lfp_field.cuh"
namespace lfp {
// The accumulator bound.  acc160_bias16 covers the 16 subtracted products of ONE negacyclic product.  A coefficient of a sum over n_terms <= 64 products subtracts
// up to 15 * 64 = 960 of them, each below p^2 < p 2^64: the sum starts from 1024 p 2^64, a multiple of p 2^64 (it vanishes in the reduction) that 960 subtracted
// products cannot exhaust, and with all 16 * 64 = 1024 products added stays below 2048 p 2^64 < 2^139 -- far inside the 160 bits, whatever n_terms is.
__device__ __forceinline__ void acc160_bias1024(Acc160 &n) { n.a[0] = n.a[1] = 0; n.a[2] = (u32)(P << 10); n.a[3] = (u32)((P << 10) >> 32); n.a[4] = (u32)(P >> 54); }
// n += coefficient c of xM * y: xM 16 Montgomery words, y 16 canonical words (both LDS); the wrapped terms enter with a minus sign
__device__ __forceinline__ void ring_mac16(Acc160 &n, const u64 *xM, const u64 *y, u32 c) {
#pragma unroll
    for (u32 j = 0; j < 16; j++) acc160_mad_signed(n, xM[j], y[(c - j) & 15], j > c);
}
template <int MODE>
__global__ void __launch_bounds__(256) k_ring_mul(const u64 *a, const u64 *b, u32 n_terms, u64 count, u64 *out, u32 *flag) {      // (no __restrict__: out may be a or b)
    __shared__ __attribute__((aligned(16))) u64 sbuf[2][512];                        // [buffer][operand half][element][word]
    __shared__ __attribute__((aligned(16))) u64 sbM[MODE ? 64 * 16 : 16];            // mode 1: the n_terms coefficients, Montgomery (<= 8 KB)
    const u32 tid = threadIdx.x, c = tid & 15, pl = tid >> 4, which = tid >> 7, q = tid & 127;
    const u64 groups = (count + 15) / 16;
    if (blockIdx.x >= groups) return;                                                // (the launcher starts no such workgroup)
    if (MODE)
        for (u32 i = tid; i < n_terms * 16; i += 256) sbM[i] = b[i];                 // (visible behind the first barrier; every workgroup passes one)
    bool bad = false;
    // the pair this lane loads in step (g, i): pair q & 7 of element q >> 3 of the group, from the operand of its half
    auto fetch = [&](u64 g, u32 i) {
        const u64 e = g * 16 + (q >> 3);
        const u32 t = MODE ? i + which : i;
        ulonglong2 v = make_ulonglong2(0, 0);
        if (e < count && t < n_terms) {
            const u64 *src = (MODE || !which) ? a : b;
            v = *(const ulonglong2 *)(src + ((u64)t * count + e) * 16 + 2 * (q & 7));
            bad |= v.x >= P || v.y >= P;
        }
        return v;
    };
    constexpr u32 STEP = MODE ? 2 : 1;
    u64 g = blockIdx.x;
    u32 i = 0, buf = 0;
    ulonglong2 v = fetch(g, 0);
    Acc160 n;
    acc160_bias1024(n);
    for (;;) {
        if (!MODE && !which) { v.x = to_mont(v.x); v.y = to_mont(v.y); }
        *(ulonglong2 *)&sbuf[buf][which * 256 + 2 * q] = v;
        u64 g2 = g;
        u32 i2 = i + STEP;
        if (i2 >= n_terms) { i2 = 0; g2 = g + gridDim.x; }
        const bool more = g2 < groups;
        if (more) v = fetch(g2, i2);
        __syncthreads();
        const u64 *s0 = sbuf[buf] + pl * 16, *s1 = s0 + 256;
        if (MODE) {
            ring_mac16(n, sbM + i * 16, s0, c);
            if (i + 1 < n_terms) ring_mac16(n, sbM + (i + 1) * 16, s1, c);
        } else ring_mac16(n, s0, s1, c);
        buf ^= 1;
        if (i2 == 0) {                                                               // the group's last step: ONE reduction, then the store
            const u64 r = acc160_red(n), r1 = __shfl_xor(r, 1);
            const u64 e = g * 16 + pl;
            if (!(c & 1) && e < count) *(ulonglong2 *)(out + e * 16 + c) = make_ulonglong2(r, r1);
            acc160_bias1024(n);
        }
        if (!more) break;
        g = g2; i = i2;
    }
    if (__any(bad) && (tid & 63) == 0) atomicOr(flag, 1u);                           // (every lane of the wave is here again: one atomic per wave that saw a bad word)
}
u32 ring_mul_blocks(u64 count, u32 cap) {
    const u64 g = (count + 15) / 16;
    return (u32)(g < 1 ? 1 : (g > cap ? cap : g));
}
void launch_ring_mul(const u64 *a, const u64 *b, u32 n_terms, u64 count, int mode, u64 *out, u32 *flag, u32 blocks, hipStream_t s) {
    if (mode) hipLaunchKernelGGL(k_ring_mul<1>, dim3(blocks), dim3(256), 0, s, a, b, n_terms, count, out, flag);
    else hipLaunchKernelGGL(k_ring_mul<0>, dim3(blocks), dim3(256), 0, s, a, b, n_terms, count, out, flag);
}
}  // namespace lfp
