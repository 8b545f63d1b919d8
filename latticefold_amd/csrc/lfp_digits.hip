// lfp_digits.hip -- gfx950 kernels of the "gadget maps on arrays" section of include/lfplus.h (lfp_digits.cpp) on the Frog ring Z_p[X]/(X^16 + 1), coefficient form:
//   k_digits_decompose  the k balanced base-b digits of every centred word (lfp::digit_step, the one digit rule of the slice), in gadget or plane order
//   k_digits_recompose  sum_i b^i in_i word by word mod p: the k products as one lazy 160-bit sum, one reduction per output word
//   k_absmax            the largest |centred word| of an array (lfplus_linf_norm; the relation checks of lfp_check.cpp)
//   k_gadget_*          a short CSR matrix over z expanded into the complete resident n x n matrix over f = G^-1 z, both orientations
// HBM-bound integer work; no MFMA.  A thread owns one (element, coefficient) word and the kernels stride over the words: a wave reads and writes four whole
// 128-byte elements per access in both layouts (the k digits of a word go to k different elements, 16 lanes abreast in each).
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include "lfp_kernels.h"
#include "lfp_dev.cuh"

namespace lfp {
static inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
static inline int log2_exact(u64 b) {      // log2(b) when b is a power of two, else -1: digit_step's shift / division switch
    if (!b || (b & (b - 1))) return -1;
    int sh = 0;
    while ((1ull << sh) != b) sh++;
    return sh;
}
u32 digit_blocks(u64 words, u32 cap) {
    const u64 b = cdiv(words, 256);
    return (u32)(b < 1 ? 1 : b > cap ? cap : b);
}
__device__ __forceinline__ u64 canon_signed(int64_t d) { return d >= 0 ? (u64)d : P - (u64)(-d); }

// estride: words between consecutive digits of one word (16 in gadget order, count * 16 in planes); jstride: words between the first digits of consecutive elements
__global__ void __launch_bounds__(256) k_digits_decompose(const u64 *in, u64 words, u64 b, int sh, u32 k, u64 estride, u64 jstride, u64 *out, u32 *flag) {
    bool bad = false;
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < words; w += (u64)gridDim.x * 256) {
        const u64 v = in[w];
        bad |= v >= P;
        int64_t cur = centre(v);
        u64 *dst = out + (w >> 4) * jstride + (w & 15);
        for (u32 i = 0; i < k; i++) dst[(u64)i * estride] = canon_signed(digit_step(cur, b, sh));
    }
    if (bad) atomicOr(flag, 1u);
}
void launch_digits_decompose(const u64 *in, u64 count, u64 b, u32 k, int layout, u64 *out, u32 *flag, u32 blocks, hipStream_t s) {
    const u64 estride = layout ? count * D : D, jstride = layout ? D : (u64)k * D;
    hipLaunchKernelGGL(k_digits_decompose, dim3(blocks), dim3(256), 0, s, in, count * D, b, log2_exact(b), k, estride, jstride, out, flag);
}

// at most 64 products below p^2 < 2^128 in the 160-bit sum; powers in Montgomery form against canonical words: acc160_red leaves the canonical sum
__global__ void __launch_bounds__(256) k_digits_recompose(const u64 *in, u64 words, u32 k, u64 estride, u64 jstride, DigitPows pw, u64 *out, u32 *flag) {
    bool bad = false;
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < words; w += (u64)gridDim.x * 256) {
        const u64 *src = in + (w >> 4) * jstride + (w & 15);
        Acc160 acc;
        acc160_zero(acc);
        for (u32 i = 0; i < k; i++) {
            const u64 v = src[(u64)i * estride];
            bad |= v >= P;
            acc160_mad(acc, pw.pM[i], v);
        }
        out[w] = acc160_red(acc);
    }
    if (bad) atomicOr(flag, 1u);
}
void launch_digits_recompose(const u64 *in, u64 count, u32 k, int layout, const DigitPows &pw, u64 *out, u32 *flag, u32 blocks, hipStream_t s) {
    const u64 estride = layout ? count * D : D, jstride = layout ? D : (u64)k * D;
    hipLaunchKernelGGL(k_digits_recompose, dim3(blocks), dim3(256), 0, s, in, count * D, k, estride, jstride, pw, out, flag);
}

__global__ void __launch_bounds__(256) k_absmax(const u64 *x, size_t words, u64 *absmax, u32 *flag) {
    u64 mx = 0;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
        const u64 v = x[i];
        bad |= v >= P;
        const u64 a = abs_centred(v);
        mx = a > mx ? a : mx;
    }
    wave_atomic_max(mx, absmax);
    if (flag && bad) atomicOr(flag, 1u);
}
void launch_absmax(const u64 *x, size_t words, u64 *absmax, hipStream_t s, u32 *flag) {
    size_t b = cdiv(words, 256 * 8);
    b = b < 1 ? 1 : (b > 2048 ? 2048 : b);
    hipLaunchKernelGGL(k_absmax, dim3((unsigned)b), dim3(256), 0, s, x, words, absmax, flag);
}

// ---- the gadget form of a short CSR matrix -----------------------------------------------------------------------------------------------
// rowptr[r] = k rowptr_s[min(r, rows)] for r <= n (rows from `rows` on are empty); colptr[j k + i] = k colptr_s[j] + i (colptr_s[j + 1] - colptr_s[j]), colptr[n] = k nnz
__global__ void __launch_bounds__(256) k_gadget_ptrs(const u32 *rowptr_s, const u32 *colptr_s, u64 rows, u64 m, u64 n, u32 k, u32 *rowptr, u32 *colptr) {
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r <= n; r += (u64)gridDim.x * 256) {
        rowptr[r] = k * rowptr_s[r < rows ? r : rows];
        const u64 j = r / k, i = r - j * k;
        colptr[r] = r == n ? k * colptr_s[m] : k * colptr_s[j] + (u32)i * (colptr_s[j + 1] - colptr_s[j]);
    }
}
// thread = (entry e in CSR order, coefficient t): col, valM (Montgomery) and valMc of the k entries e k + i
__global__ void __launch_bounds__(256) k_gadget_csr(const u32 *col_s, const u64 *val_s, u64 nnz, u32 k, DigitPows pw, GadgetOut o) {
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nnz * D; w += (u64)gridDim.x * 256) {
        const u64 e = w >> 4;
        const u32 t = (u32)(w & 15), c = col_s[e];
        const u64 v = val_s[w];
        for (u32 i = 0; i < k; i++) {
            const u64 d = e * k + i, vm = to_mont(mont_mul(v, pw.pM[i]));
            o.valM[d * D + t] = vm;
            if (t == 0) {
                o.col[d] = c * k + i;
                if (o.valMc) o.valMc[d] = vm;
            }
        }
    }
}
// thread = (position pos of the short CSC order, coefficient t): rowidx, valT (canonical) and valTc of the k entries k colptr_s[j] + i cnt_j + (pos - colptr_s[j]).
// The row of entry e is found in rowptr_s (the last r with rowptr_s[r] <= e)
__global__ void __launch_bounds__(256) k_gadget_csc(const u32 *rowptr_s, const u32 *col_s, const u64 *val_s, const u32 *colptr_s, const u32 *perm, u64 rows, u64 nnz, u32 k,
                                                    DigitPows pw, GadgetOut o) {
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nnz * D; w += (u64)gridDim.x * 256) {
        const u64 pos = w >> 4;
        const u32 t = (u32)(w & 15), e = perm[pos], j = col_s[e];
        const u64 c0 = colptr_s[j], cnt = colptr_s[j + 1] - c0, v = val_s[(u64)e * D + t];
        u64 lo = 0, hi = rows;      // rowptr_s[lo] <= e < rowptr_s[hi]
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (rowptr_s[mid] <= e) lo = mid; else hi = mid;
        }
        for (u32 i = 0; i < k; i++) {
            const u64 d = (u64)k * c0 + (u64)i * cnt + (pos - c0), vc = mont_mul(v, pw.pM[i]);
            o.valT[d * D + t] = vc;
            if (t == 0) {
                o.rowidx[d] = (u32)lo;
                if (o.valTc) o.valTc[d] = vc;
            }
        }
    }
}
__global__ void __launch_bounds__(256) k_iota(u32 *x, u64 n) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) x[i] = (u32)i;
}
static inline unsigned key_bits(u64 m) {
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) < m) bits++;
    return bits;
}
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// tmp: the identity | the sorted keys | the sort's own storage
size_t gadget_perm_bytes(u64 nnz, u64 m) {
    size_t st = 0;
    (void)rocprim::radix_sort_pairs(nullptr, st, (const u32 *)nullptr, (u32 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, (size_t)nnz, 0u, key_bits(m), (hipStream_t) nullptr);
    return 2 * align256(nnz * 4) + align256(st ? st : 1);
}
hipError_t launch_gadget_perm(const u32 *col_s, u64 nnz, u64 m, u32 *perm, void *tmp, size_t tmp_bytes, hipStream_t s) {
    u32 *iota = (u32 *)tmp, *keys = (u32 *)((char *)tmp + align256(nnz * 4));
    void *store = (char *)tmp + 2 * align256(nnz * 4);
    size_t st = tmp_bytes - 2 * align256(nnz * 4);
    hipLaunchKernelGGL(k_iota, dim3(digit_blocks(nnz, 2048)), dim3(256), 0, s, iota, nnz);
    // (a radix sort is stable: the entries of a column keep their CSR order, rows ascending)
    return rocprim::radix_sort_pairs(store, st, col_s, keys, (const u32 *)iota, perm, (size_t)nnz, 0u, key_bits(m), s);
}
void launch_gadget_expand(const u32 *rowptr_s, const u32 *col_s, const u64 *val_s, const u32 *colptr_s, const u32 *perm, u64 rows, u64 m, u64 n, u64 nnz, u32 k,
                          const DigitPows &pw, const GadgetOut &o, hipStream_t s) {
    hipLaunchKernelGGL(k_gadget_ptrs, dim3(digit_blocks(n + 1, 2048)), dim3(256), 0, s, rowptr_s, colptr_s, rows, m, n, k, o.rowptr, o.colptr);
    if (!nnz) return;
    hipLaunchKernelGGL(k_gadget_csr, dim3(digit_blocks(nnz * D, 2048)), dim3(256), 0, s, col_s, val_s, nnz, k, pw, o);
    hipLaunchKernelGGL(k_gadget_csc, dim3(digit_blocks(nnz * D, 2048)), dim3(256), 0, s, rowptr_s, col_s, val_s, colptr_s, perm, rows, nnz, k, pw, o);
}
}  // namespace lfp
