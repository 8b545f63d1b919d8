// lfp_dev.cuh -- device helpers shared by the kernel files of the LatticeFold+ slice (lfp_kernels.hip, lfp_ingest.hip, lfp_check.hip, lfp_digits.hip): the balanced
// digit rule, centred representatives and their wave-wide maximum, the word-wise reduction mod p and the block-level sum over the 16 row lanes
#pragma once
#include "lfp_field.cuh"
namespace lfp {
// (r 2^64 + w) mod p for r < p: mont_mul(r, 2^128) = r 2^64
__device__ __forceinline__ u64 red_word(u64 r, u64 w) { return add_p(mont_mul(r, R2), w >= P ? w - P : w); }

// balanced digit step (stark_rings::balanced_decomposition as restated in oracle/lfp.c: truncating remainder, |rem| <= b/2 kept)
__device__ __forceinline__ int64_t digit_step(int64_t &cur, u64 b, int sh) {
    int64_t q, rem;
    if (sh >= 0) {
        q = (cur + ((cur >> 63) & (int64_t)(b - 1))) >> sh;
        rem = cur - (q << sh);
    } else {
        q = cur / (int64_t)b;
        rem = cur - q * (int64_t)b;
    }
    int64_t half = (int64_t)(b >> 1), ar = rem < 0 ? -rem : rem;
    if (ar > half) {
        if (rem < 0) { rem += (int64_t)b; q -= 1; }
        else { rem -= (int64_t)b; q += 1; }
    }
    cur = q;
    return rem;
}
__device__ __forceinline__ int64_t centre(u64 v) { return v <= (P - 1) / 2 ? (int64_t)v : -(int64_t)(P - v); }
// |centred w| for a canonical word: w if w <= (p - 1) / 2, else p - w
__device__ __forceinline__ u64 abs_centred(u64 w) { return w <= (P - 1) / 2 ? w : P - w; }
// the wave's maximum -> one vector atomicMax on a 64-bit word (skipped when it cannot raise a zero-initialised word)
__device__ __forceinline__ void wave_atomic_max(u64 v, u64 *dst) {
    for (int o = 32; o; o >>= 1) {
        const u64 x = __shfl_xor(v, o);
        v = x > v ? x : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax((unsigned long long *)dst, (unsigned long long)v);
}

// sum over the 16 row lanes (tid >> 4) of a value mod p held by thread (jl, t): two 16-lane shuffles inside each wave, LDS across waves;
// valid in threads tid < 16
__device__ __forceinline__ u64 sum_over_row_lanes(u64 v, u64 (*sh)[16], int tid) {
    v = add_p(v, __shfl_xor(v, 16));
    v = add_p(v, __shfl_xor(v, 32));
    __syncthreads();
    if ((tid & 63) < 16) sh[tid >> 6][tid & 15] = v;
    __syncthreads();
    u64 r = 0;
    if (tid < 16) r = add_p(add_p(sh[0][tid], sh[1][tid]), add_p(sh[2][tid], sh[3][tid]));
    return r;
}
}  // namespace lfp
