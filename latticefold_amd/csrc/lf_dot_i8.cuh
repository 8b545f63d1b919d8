// lf_dot_i8.cuh -- what the two inner-product translation units (lf_dot_i8.hip: Goldilocks, 64-bit words, F_{p^3} slots; bb_dot_i8.hip: BabyBear, centred 32-bit
// Montgomery words, F_{p^9} slots) share besides lf_i8_mma.cuh: the Y digit pack, the GEMM kernels' argument struct and operand loads, the sum over the column chunks and the host's plan
// of a call.  The GEMM kernels k_dot_i8 and k_bbdot_i8 stay in their files.
#pragma once
#include <type_traits>

#include "lf_i8_launch.h"
#include "lf_i8_mma.cuh"

namespace i8mma {
#if defined(__HIPCC__)   // (the kernels: not for the stand-alone host program that includes this file for DotPlan, lf_q_pack_selftest.cpp)
// W = word of the ring (D = sizeof(W) balanced digits), COMP = words per slot (3 / 9): 8 COMP word planes per vector, 3 COMP D digit rows per slot.
// YB[slot][(b*COMP + cq)*D + v][.] = digit v of Y_b[COMP slot + cq][i] in the operand order of a K-step (kstep_col) per block of 64 columns, zero beyond n and
// below `lead` (those columns belong to the neighbour slice); ldq columns per row; wave = (word plane, 8 blocks of 64 columns)
template <class W, uint32_t COMP>
__global__ void __launch_bounds__(256) k_dot_pack_y(const W *Y, size_t ldy, uint32_t nb, size_t n, size_t lead, size_t ldq, unsigned char *YB) {
    typedef typename std::conditional<sizeof(W) == 8, uint64_t, uint32_t>::type U;
    constexpr uint32_t D = sizeof(W), PLANES = 8 * COMP, PER_WAVE = 8;   // blocks of 64 columns per wave
    __shared__ U sm[4][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t blocks = ldq / 64, groups = (blocks + PER_WAVE - 1) / PER_WAVE, wid = (size_t)blockIdx.x * 4 + wave;
    if (wid >= (size_t)nb * PLANES * groups) return;             // (no block-wide barrier below: a wave only reads what it wrote)
    const uint32_t wp = (uint32_t)(wid / groups);                 // word plane b*PLANES + COMP*slot + cq
    const uint32_t b = wp / PLANES, slot = (wp % PLANES) / COMP, cq = wp % COMP;
    const W *src_row = Y + ((size_t)b * PLANES + COMP * slot + cq) * ldy;
    unsigned char *dst_rows = YB + ((size_t)slot * (3 * COMP * D) + (b * COMP + cq) * D) * ldq;
    const uint32_t v = lane / (64 / D), c0 = D * (lane % (64 / D));   // lane L writes digit plane v, operand positions c0 .. c0 + D - 1
    const unsigned char *src = (const unsigned char *)&sm[wave][0];
    for (uint32_t k = 0; k < PER_WAVE; k++) {
        const size_t blk = (wid % groups) * PER_WAVE + k;
        if (blk >= blocks) break;
        const size_t i0 = blk * 64, i = i0 + lane;
        sm[wave][lane] = (i >= lead && i < n) ? balanced_bytes((U)src_row[i]) : 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        U o = 0;
#pragma unroll
        for (int t = 0; t < (int)D; t++) {
            const uint32_t col = kstep_col(c0 + t);
            o |= (U)src[col * D + v] << (8 * t);
        }
        *(U *)(dst_rows + (size_t)v * ldq + i0 + c0) = o;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}
// the arguments of a GEMM kernel (k_dot_i8 / k_bbdot_i8); COMP words per slot, D digits per word
template <class W>
struct DotArgs {
    const W *X;                 // [na][8 COMP][ldx]
    size_t ldx, n;
    uint32_t na;                // <= 16
    const unsigned char *YB;    // [8][3 COMP D][ldq]
    size_t ldq;
    uint32_t nrows_y;           // COMP D nb
    uint32_t nsteps, steps_per_chunk, chunks;
    int32_t *part;              // [unit 8 COMP][chunk][digit u][column tile][64][4]
};
// The 16 words of a lane in the inner-dimension order of a K-step (kstep_col: one lane = 128 contiguous bytes ran at 2 TB/s, L1-tag-bound), two adjacent words
// per load (rows of X start on two-word boundaries only: DotPlan's lead column); k_dot_pack_y stores the Y digits in the same order
template <class W, class U>
__device__ __forceinline__ void dot_load_x(const W *xrow, size_t iw, uint32_t g, size_t n, bool xlive, U (&dst)[16]) {
    typedef typename std::conditional<sizeof(W) == 8, ulonglong2, int2>::type W2;
    if (xlive && iw + 64 <= n) {
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const W2 p = *(const W2 *)(xrow + iw + 8 * t + 2 * g);
            dst[2 * t] = (U)p.x; dst[2 * t + 1] = (U)p.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const size_t i = kstep_col(iw, g, e);
            dst[e] = (xlive && i < n) ? (U)xrow[i] : 0;
        }
    }
}
// the NT column tiles of packed Y digits of a K-step: 16 bytes per lane and tile, zero rows beyond nrows_y
template <int NT>
__device__ __forceinline__ void dot_load_y(const unsigned char *yb, size_t ldq, size_t i0, uint32_t row, uint32_t nrows_y, v4i (&b)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const uint32_t r = 16 * nt + row;
        b[nt] = r < nrows_y ? *(const v4i *)(yb + (size_t)r * ldq + i0) : v4i{0, 0, 0, 0};
    }
}
// tot[unit][e] = sum over the chunks (64-bit) of part[unit][chunk][e], e < PER (the int32 accumulators of one wave of the GEMM kernel); grid (PER / 256, units)
template <uint32_t PER>
__global__ void __launch_bounds__(256) k_dot_sum(const int32_t *part, uint32_t chunks, long long *tot) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x, unit = blockIdx.y;
    long long s = 0;
    for (uint32_t ch = 0; ch < chunks; ch++) s += part[((size_t)unit * chunks + ch) * PER + e];
    tot[(size_t)unit * PER + e] = s;
}
#endif
// The column plan of one call.  A slice whose first word is not aligned for the GEMM kernel's two-word loads (a rank's slice of a sharded step) starts `lead` = 1
// column early, and that column gets zero digits on the Y side.  `want` chunks of K-steps fill the chip in one batch (one wave per SIMD); the chunk count is not
// monotone in the step count (80 steps -> 40 chunks, 81 -> 27), so the scratch is sized for `want`.
struct DotPlan {
    size_t lead, n, ldq;                       // n: columns including the lead; ldq: n padded to K-steps of 64
    uint32_t nsteps, chunks, steps_per_chunk;
    // false: the shape is not handled (fewer than 64 columns, words not aligned, or a wave's int32 accumulators could overflow)
    template <class W>
    bool make(const W *X, size_t n_, uint32_t want) {
        if (n_ < 64 || ((size_t)X % sizeof(W))) return false;
        lead = ((size_t)X % (2 * sizeof(W))) / sizeof(W);
        n = n_ + lead;
        ldq = cdiv(n, 64) * 64;
        nsteps = (uint32_t)(ldq / 64);
        chunks = (uint32_t)cdiv(nsteps, cdiv(nsteps, want < nsteps ? want : nsteps));
        steps_per_chunk = (uint32_t)cdiv(nsteps, chunks);
        return steps_per_chunk < 2048;         // exactness: a wave adds steps_per_chunk * 64 digit products of at most 2^14 into an int32 accumulator
    }
    template <class A, class W>   // A: the kernel's argument struct, a DotArgs<W> under the kernel's own name
    A args(const W *X, size_t ldx, uint32_t na, const unsigned char *YB, uint32_t nrows_y, int32_t *part) const {
        A a;
        a.X = X - lead; a.ldx = ldx; a.n = n; a.na = na; a.YB = YB; a.ldq = ldq; a.nrows_y = nrows_y;
        a.nsteps = nsteps; a.chunks = chunks; a.steps_per_chunk = steps_per_chunk; a.part = part;
        return a;
    }
    // grid of the pack kernel: one wave per (word plane, 8 K-steps), four waves per block
    unsigned pack_blocks(uint32_t nb, uint32_t planes) const { return (unsigned)cdiv((size_t)nb * planes * cdiv(nsteps, 8), 4); }
};
}  // namespace i8mma
