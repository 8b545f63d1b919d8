// lf_witness_parts.hip -- decompose_witness (nifs/decomposition.rs:162-167) on witness handles: the int32 coefficient planes of a witness cut into K planes of
// balanced base-b digits, one allocation per part (k_witness_cut), and K such planes joined into the witness they are the parts of, refused unless they are
// exactly what the cut would produce from their sum (k_witness_join).  Both are streams over a flat array of RE * N coefficients: 4 B in and 4 K B out per
// coefficient (the join: the other way round), no LDS.  A thread takes four consecutive coefficients as one 16-byte access, so a wave reads and writes 1 KiB
// runs; the array length need not be a multiple of four (the last total % 4 coefficients go one by one).
#include "lf_witness_parts.h"

#include "lf_i8g_dec.cuh"

namespace lfparts {
namespace {

struct PartPtrs { int32_t *p[MAX_PARTS]; };

// the chain of lf_i8g_dec.cuh started from a centred integer instead of a residue
__device__ __forceinline__ void seed(lfdec::DigitChain &ch, int64_t v) {
    ch.neg = v < 0;
    ch.mag = ch.neg ? 0 - (uint64_t)v : (uint64_t)v;
    ch.cur = v;
}
// what is left of the value after the last digit: zero iff the K digits are the whole decomposition
__device__ __forceinline__ bool carry_left(const lfdec::DigitChain &ch, uint32_t lb, int mode) { return mode == 1 && lb > 1 ? ch.cur != 0 : ch.mag != 0; }

__global__ void __launch_bounds__(256) k_witness_cut(const int32_t *planes, size_t total, uint32_t K, uint32_t lb, int mode, PartPtrs out) {
    const size_t nv = total / 4;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < nv; g += (size_t)gridDim.x * 256) {
        const int4 v = ((const int4 *)planes)[g];
        lfdec::DigitChain ch[4];
        seed(ch[0], v.x); seed(ch[1], v.y); seed(ch[2], v.z); seed(ch[3], v.w);
        for (uint32_t k = 0; k < K; k++) {
            int4 d;
            d.x = (int32_t)ch[0].next(lb, mode); d.y = (int32_t)ch[1].next(lb, mode); d.z = (int32_t)ch[2].next(lb, mode); d.w = (int32_t)ch[3].next(lb, mode);
            ((int4 *)out.p[k])[g] = d;
        }
    }
    const size_t i = nv * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < total) {
        lfdec::DigitChain ch;
        seed(ch, planes[i]);
        for (uint32_t k = 0; k < K; k++) out.p[k][i] = (int32_t)ch.next(lb, mode);
    }
}

// one coefficient of the join.  Pass 1 (add): a digit outside [lo, hi] is flagged and counts as zero, so |sum| < 2^(lb K + 1) never wraps.  Pass 2 (cmp): the
// chain restarted from the sum must give back every digit
struct Join {
    int64_t sum = 0;
    uint32_t bad = 0;
    __device__ __forceinline__ void add(int32_t d, uint32_t k, uint32_t lb, int32_t lo, int32_t hi) {
        if (d < lo || d > hi) { bad |= FLAG_DIGIT; d = 0; }
        sum += (int64_t)d * ((int64_t)1 << (lb * k));
    }
    __device__ __forceinline__ int32_t finish(lfdec::DigitChain &ch, uint32_t lb, int mode, uint64_t bound) {
        if (carry_left(ch, lb, mode)) bad |= FLAG_NOT_CANONICAL;
        const uint64_t mag = sum < 0 ? 0 - (uint64_t)sum : (uint64_t)sum;
        if (mag > bound) bad |= FLAG_NORM;                        // the bound rule of k_coef_to_i32
        else if (sum > 0x7fffffffll) bad |= FLAG_NO_I32;
        return bad ? 0 : (int32_t)sum;
    }
};

__global__ void __launch_bounds__(256) k_witness_join(PartPtrs in, size_t total, uint32_t K, uint32_t lb, int mode, uint64_t bound, int32_t *planes, uint32_t *flag) {
    const int32_t half = 1 << (lb - 1), lo = -half, hi = mode == 1 && lb > 1 ? half - 1 : half;
    const size_t nv = total / 4;
    uint32_t bad = 0;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < nv; g += (size_t)gridDim.x * 256) {
        Join j[4];
        for (uint32_t k = 0; k < K; k++) {
            const int4 d = ((const int4 *)in.p[k])[g];
            j[0].add(d.x, k, lb, lo, hi); j[1].add(d.y, k, lb, lo, hi); j[2].add(d.z, k, lb, lo, hi); j[3].add(d.w, k, lb, lo, hi);
        }
        lfdec::DigitChain ch[4];
#pragma unroll
        for (int q = 0; q < 4; q++) seed(ch[q], j[q].sum);
        for (uint32_t k = 0; k < K; k++) {   // (the wave reads again the lines it has just loaded)
            const int4 d = ((const int4 *)in.p[k])[g];
            if (ch[0].next(lb, mode) != d.x) j[0].bad |= FLAG_NOT_CANONICAL;
            if (ch[1].next(lb, mode) != d.y) j[1].bad |= FLAG_NOT_CANONICAL;
            if (ch[2].next(lb, mode) != d.z) j[2].bad |= FLAG_NOT_CANONICAL;
            if (ch[3].next(lb, mode) != d.w) j[3].bad |= FLAG_NOT_CANONICAL;
        }
        int4 o;
        o.x = j[0].finish(ch[0], lb, mode, bound); o.y = j[1].finish(ch[1], lb, mode, bound);
        o.z = j[2].finish(ch[2], lb, mode, bound); o.w = j[3].finish(ch[3], lb, mode, bound);
        ((int4 *)planes)[g] = o;
        bad |= j[0].bad | j[1].bad | j[2].bad | j[3].bad;
    }
    const size_t i = nv * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < total) {
        Join j;
        for (uint32_t k = 0; k < K; k++) j.add(in.p[k][i], k, lb, lo, hi);
        lfdec::DigitChain ch;
        seed(ch, j.sum);
        for (uint32_t k = 0; k < K; k++)
            if (ch.next(lb, mode) != in.p[k][i]) j.bad |= FLAG_NOT_CANONICAL;
        planes[i] = j.finish(ch, lb, mode, bound);
        bad |= j.bad;
    }
    // one vector atomic per wave that saw a violation, by its lowest lane (every lane arrives here: the ballots see whole waves)
    uint32_t wave_bad = 0;
#pragma unroll
    for (uint32_t bit = 1; bit <= FLAG_NOT_CANONICAL; bit <<= 1)
        if (__ballot(bad & bit)) wave_bad |= bit;
    if (wave_bad && (threadIdx.x & 63) == 0) atomicOr(flag, wave_bad);
}

unsigned grid_of(size_t total) {
    const size_t g = (total / 4 + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool fill(PartPtrs &a, const int32_t *const *parts, uint32_t K) {
    for (uint32_t k = 0; k < MAX_PARTS; k++) {
        a.p[k] = k < K ? (int32_t *)parts[k] : nullptr;
        if (k < K && (!parts[k] || !aligned16(parts[k]))) return false;
    }
    return true;
}

}  // namespace

int launch_witness_cut(const int32_t *planes, size_t total, uint32_t K, uint32_t lb, int mode, int32_t *const *parts, hipStream_t s) {
    PartPtrs a;
    if (!total || !K || K > MAX_PARTS || lb < 1 || lb > 16 || !planes || !aligned16(planes) || !fill(a, parts, K)) return -1;
    hipLaunchKernelGGL(k_witness_cut, dim3(grid_of(total)), dim3(256), 0, s, planes, total, K, lb, mode, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_witness_join(const int32_t *const *parts, size_t total, uint32_t K, uint32_t lb, int mode, uint64_t bound, int32_t *planes, uint32_t *flag,
                        hipStream_t s) {
    PartPtrs a;
    if (!total || !K || K > MAX_PARTS || lb < 1 || lb > 16 || K * lb > 60 || !planes || !aligned16(planes) || !flag || !fill(a, parts, K)) return -1;
    hipLaunchKernelGGL(k_witness_join, dim3(grid_of(total)), dim3(256), 0, s, a, total, K, lb, mode, bound, planes, flag);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lfparts
