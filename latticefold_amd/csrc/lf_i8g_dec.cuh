// lf_i8g_dec.cuh -- the gadget digit pass of the general commitment (lf_ajtai_i8g.hip), shared by the two ring backends: AjtaiCommitmentScheme::
// decompose_and_commit_coeff / decompose_and_commit_ntt / commit_coeff (commitment_scheme.rs:81-113).
//
// Column g = i L + l of the decomposed vector (decompose_to_vec(B, L) flattened, = lf_decompose layout 0) is digit l of the balanced base-2^lb
// decomposition of element i, coefficient-wise.  The pass writes the commit kernel's operand words for this rank's columns [col0, col0 + n) straight
// from the coefficient table: pre [NP][RD][ldw], byte q of word T = 64 + balanced base-128 digit of column col0 + 8 T + q (k_i8g_cut's cut; columns
// past n hold zero digits).  The count x L digit table is never written.  lb == 0: no decomposition, the column is the centred coefficient itself
// (commit_coeff).  A tile of 8 columns mixes elements whenever L does not divide 8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lfdec {
// The digit rule of k_decompose (lf_kernels.hip, bb_kernels.hip), digit by digit from the centred lift of a canonical residue v < p.  Mode 0: sign-magnitude,
// |digit| <= base/2, ties kept; mode 1 (base > 2): floor rule, digits in [-base/2, base/2).  The last carry is dropped, so |digit| <= base/2 for every input.
// Mode 1 forms the quotient as floor(cur / base) + (rem < 0): the same value as k_decompose's (cur - rem) >> lb wherever that difference fits an int64
// (everywhere except base 2^63 with a centred value >= 2^62, where k_decompose's difference wraps and the oracle's exact rule is kept here).
struct DigitChain {
    bool neg;
    uint64_t mag;
    int64_t cur;
    __device__ __forceinline__ void init(uint64_t v, uint64_t p) {
        neg = v > (p - 1) / 2;
        mag = neg ? p - v : v;
        cur = neg ? -(int64_t)mag : (int64_t)mag;     // |centred lift| <= (p-1)/2 < 2^63
    }
    __device__ __forceinline__ int64_t next(uint32_t lb, int mode) {
        const uint64_t mask = (1ull << lb) - 1, half = 1ull << (lb - 1);
        if (mode == 1 && lb > 1) {
            const uint64_t r0 = (uint64_t)cur & mask;
            const int64_t q0 = cur >> lb;                // floor(cur / base)
            if (r0 >= half) { cur = q0 + 1; return (int64_t)(r0 - (mask + 1)); }
            cur = q0;
            return (int64_t)r0;
        }
        const uint64_t rem = mag & mask;
        mag >>= lb;
        int64_t dg;
        if (rem > half) { dg = (int64_t)(rem - (mask + 1)); mag += 1; }
        else dg = (int64_t)rem;
        return neg ? -dg : dg;
    }
};

// One thread per (coefficient c, tile T): the 8 columns of the tile, NP digit words.  ld(off) returns the canonical residue of coefficient table entry `off`
// (element i, coefficient c at c * ldc + i).  Every column's coefficient is requested before the first digit is formed (8 independent loads, neighbours
// of one element hit the same line); the digit chain restarts where the element changes.
template <class Ld>
__global__ void __launch_bounds__(256) k_i8g_cut_dec(Ld ld, size_t ldc, uint64_t p, size_t col0, size_t n, uint32_t L, uint32_t lb, int mode, uint32_t RD,
                                                     uint32_t NP, size_t ntiles, unsigned long long *pre, size_t ldw) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= ntiles * RD) return;
    const size_t T = gid % ntiles;
    const uint32_t c = (uint32_t)(gid / ntiles);
    const size_t g0 = col0 + T * 8;
    const size_t i0 = g0 / L;
    const uint32_t l0 = (uint32_t)(g0 - i0 * L);
    uint64_t v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint32_t lq = l0 + q;
        const size_t i = i0 + lq / L;
        v[q] = T * 8 + q < n ? ld((size_t)c * ldc + i) : 0;
    }
    long long x[8];
    DigitChain ch;
    ch.init(v[0], p);
    uint32_t l = l0, kn = 0;                              // digit index of the column, digits of the chain formed so far
#pragma unroll
    for (int q = 0; q < 8; q++) {
        if (q > 0 && l == 0) { ch.init(v[q], p); kn = 0; }
        if (T * 8 + q >= n) x[q] = 0;
        else if (lb == 0) x[q] = ch.cur;
        else {
            for (; kn < l; kn++) (void)ch.next(lb, mode);  // (the tile's first column only: its element's earlier digits)
            x[q] = ch.next(lb, mode);
            kn++;
        }
        if (++l == L) l = 0;
    }
    for (uint32_t k = 0; k < NP; k++) {
        unsigned long long w = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const long long t = x[q] + 64;
            w |= (unsigned long long)(t & 127) << (8 * q);
            x[q] = t >> 7;
        }
        pre[((size_t)k * RD + c) * ldw + T] = w;
    }
}
}  // namespace lfdec
