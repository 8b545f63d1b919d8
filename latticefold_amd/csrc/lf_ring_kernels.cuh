// lf_ring_kernels.cuh -- the word-generic gfx950 kernels of both ring backends, written once: the AoS <-> plane relayout at the ABI, the witness and table
// plumbing (fill, decompose / recompose, int32 planes, l-infinity norm), the radix-2 CRT butterflies with the forward shell, and the tables and sliding
// window of the folded witness.  Each is a template over a device word policy F (the folded witness: over the ring degree), instantiated from the ring's own
// translation unit (lf_kernels.hip, bb_kernels.hip) as lf_i8g_dec.cuh's digit pass is; the launchers declared in lf_kernels.h / bb_kernels.h forward to the
// launchers here.  This header includes no ring header.
//
// The policy (lf::GoldF in lf_kernels_dev.cuh, lfbb::BbF in bb_kernels_dev.cuh):
//   word                    the device word (u64 canonical / int32 centred Montgomery)
//   RE, TAU                 words per ring element, extension degree of a slot
//   P, to_canon             the prime, and word -> canonical residue, in the width of the ring's residues (u64 / u32: the 31-bit ring keeps its 32-bit
//                           compares and subtractions); to_canon is the identity on Goldilocks
//   from_canon              u64 -> word (the identity on Goldilocks)
//   add, sub, mul, one      field arithmetic on words
//   from_i64                a centred small integer as a word
//   splitmix                the ring's SplitMix64 sampler (canonical residue)
//   XbMat, xb_slot_pass     the matrix of an external basis of F_{p^TAU} and its product with the 64 x 8 slots of a tile in LDS
// Kernels with an extension-field product or a lazy accumulator (eq, SpMV, inner products, fix, the round and commit kernels) differ in schedule, not only
// in the word, and stay per ring.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace lfk {

typedef uint64_t u64;
typedef uint32_t u32;

static inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }
static inline unsigned grid_for(size_t n, unsigned cap = 2048) {
    size_t g = (n + 255) / 256;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

// ---------------------------------------------------------------------------------------------------------
// layout (+ the conversion of the ring's device word at the ABI): tile of 64 elements x RE words through LDS, the odd row length keeps a pass on distinct banks
// CHECKED: the source is a caller's own device buffer (the _dev entry points), read in place, and every word is validated: a wave that saw a word >= p sets
// *flag -- one vector atomic by its lowest lane after a ballot (every lane of the block runs the same trips, so the ballot sees whole waves)
// UNLESS: the result of a _dev call into the caller's buffer: nothing is written when the checked relayout of the call's input raised *flag
// XBASIS: the context is in an external basis of F_{p^TAU} (lf_set_ext_basis).  Between the two passes over the tile every (element, slot) is multiplied by the
// matrix M (F::xb_slot_pass), in place in the tile: M = T^-1 on the way in, after the canonical test has seen the caller's own words, M = T on the way out,
// before the AoS write.
// ELEM (aos_to_soa only): the destination is element-major device words [n][RE] (launch_aos_words: the operand k_spmv_t gathers whole elements from) instead of
// the plane table -- the same tile, canonical test and basis pass, only the store differs.
// Opt: the kernel arguments behind (src, dst, n) -- the flag word if CHECKED / UNLESS, then the matrix (by value: wave-uniform) if XBASIS.  Only what an
// instantiation reads is passed; opt_arg picks by type.
template <class T, class U, class... Rest>
__device__ __forceinline__ const T &opt_arg(const U &u, const Rest &...rest) {
    if constexpr (std::is_same<T, U>::value) return u;
    else return opt_arg<T>(rest...);
}
template <class F, bool CHECKED, bool XBASIS, bool ELEM = false>
__device__ __forceinline__ void aos_to_soa_tile(const u64 *aos, typename F::word *soa, size_t n, u32 *flag, const typename F::XbMat *M) {
    constexpr int RE = F::RE;
    __shared__ typename F::word tile[64][RE + 1];
    size_t base = (size_t)blockIdx.x * 64;
    bool bad = false;
    for (int idx = threadIdx.x; idx < 64 * RE; idx += 256) {
        size_t e = base + idx / RE;
        const u64 v = e < n ? aos[e * RE + idx % RE] : 0;
        if (CHECKED) bad |= v >= F::P;
        tile[idx / RE][idx % RE] = F::from_canon(v);
    }
    if (CHECKED) {
        if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
    }
    __syncthreads();
    if (XBASIS) {
        F::xb_slot_pass(tile, *M);
        __syncthreads();
    }
    if constexpr (ELEM) {
        for (int idx = threadIdx.x; idx < 64 * RE; idx += 256) {
            const size_t e = base + idx / RE;
            if (e < n) soa[e * RE + idx % RE] = tile[idx / RE][idx % RE];
        }
        return;
    }
    for (int idx = threadIdx.x; idx < 64 * RE; idx += 256) {
        int w = idx / 64, j = idx % 64;
        if (base + j < n) soa[(size_t)w * n + base + j] = tile[j][w];
    }
}
template <class F, bool XBASIS>
__device__ __forceinline__ void soa_to_aos_tile(const typename F::word *soa, u64 *aos, size_t n, const typename F::XbMat *M) {
    constexpr int RE = F::RE;
    __shared__ typename F::word tile[64][RE + 1];
    size_t base = (size_t)blockIdx.x * 64;
    for (int idx = threadIdx.x; idx < 64 * RE; idx += 256) {
        int w = idx / 64, j = idx % 64;
        tile[j][w] = base + j < n ? soa[(size_t)w * n + base + j] : 0;
    }
    __syncthreads();
    if (XBASIS) {
        F::xb_slot_pass(tile, *M);
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < 64 * RE; idx += 256) {
        size_t e = base + idx / RE;
        if (e < n) aos[e * RE + idx % RE] = F::to_canon(tile[idx / RE][idx % RE]);   // (Goldilocks: the tile word as it is)
    }
}
template <class F, bool CHECKED, bool XBASIS, bool ELEM = false, class... Opt>
__global__ void __launch_bounds__(256) k_aos_to_soa(const u64 *aos, typename F::word *soa, size_t n, Opt... opt) {
    static_assert(sizeof...(Opt) == (CHECKED ? 1 : 0) + (XBASIS ? 1 : 0), "flag if CHECKED, matrix if XBASIS");
    u32 *flag = nullptr;
    const typename F::XbMat *M = nullptr;
    if constexpr (CHECKED) flag = opt_arg<u32 *>(opt...);
    if constexpr (XBASIS) M = &opt_arg<typename F::XbMat>(opt...);
    aos_to_soa_tile<F, CHECKED, XBASIS, ELEM>(aos, soa, n, flag, M);
}
template <class F, bool UNLESS, bool XBASIS, class... Opt>
__global__ void __launch_bounds__(256) k_soa_to_aos(const typename F::word *soa, u64 *aos, size_t n, Opt... opt) {
    static_assert(sizeof...(Opt) == (UNLESS ? 1 : 0) + (XBASIS ? 1 : 0), "flag if UNLESS, matrix if XBASIS");
    if constexpr (UNLESS) {
        if (*opt_arg<const u32 *>(opt...)) return;
    }
    const typename F::XbMat *M = nullptr;
    if constexpr (XBASIS) M = &opt_arg<typename F::XbMat>(opt...);
    soa_to_aos_tile<F, XBASIS>(soa, aos, n, M);
}
// [n][RE] canonical u64 -> [RE][n] words; flag: the checked form, Ti: T^-1 of a context in an external basis
template <class F>
void launch_aos_to_soa(const u64 *aos, typename F::word *soa, size_t n, hipStream_t s, u32 *flag, const typename F::XbMat *Ti) {
    if (!n) return;
    const dim3 g(cdiv(n, 64)), b(256);
    if (flag && Ti) hipLaunchKernelGGL((k_aos_to_soa<F, true, true>), g, b, 0, s, aos, soa, n, flag, *Ti);
    else if (flag) hipLaunchKernelGGL((k_aos_to_soa<F, true, false>), g, b, 0, s, aos, soa, n, flag);
    else if (Ti) hipLaunchKernelGGL((k_aos_to_soa<F, false, true>), g, b, 0, s, aos, soa, n, *Ti);
    else hipLaunchKernelGGL((k_aos_to_soa<F, false, false>), g, b, 0, s, aos, soa, n);
}
template <class F>
void launch_soa_to_aos(const typename F::word *soa, u64 *aos, size_t n, hipStream_t s, const u32 *unless_flag, const typename F::XbMat *T) {
    if (!n) return;
    const dim3 g(cdiv(n, 64)), b(256);
    if (unless_flag && T) hipLaunchKernelGGL((k_soa_to_aos<F, true, true>), g, b, 0, s, soa, aos, n, unless_flag, *T);
    else if (unless_flag) hipLaunchKernelGGL((k_soa_to_aos<F, true, false>), g, b, 0, s, soa, aos, n, unless_flag);
    else if (T) hipLaunchKernelGGL((k_soa_to_aos<F, false, true>), g, b, 0, s, soa, aos, n, *T);
    else hipLaunchKernelGGL((k_soa_to_aos<F, false, false>), g, b, 0, s, soa, aos, n);
}

// An extension-field table [TAU][n] (an eq table) -> the caller's own device buffer [n][TAU] canonical u64: the store of lf_build_eq_dev, the shape of the host
// transposition of lf_build_eq.  One thread per entry: the TAU plane reads of a wave are TAU full runs, its writes one run of 64 * TAU words.  XBASIS and
// Opt as above: entry -> M * entry (M = T, internal -> external coordinates) before the write.  (No UNLESS form: the call has no device input to test.)
template <class F, bool XBASIS, class... Opt>
__global__ void __launch_bounds__(256) k_ext_to_aos(const typename F::word *soa, u64 *aos, size_t n, Opt... opt) {
    static_assert(sizeof...(Opt) == (XBASIS ? 1 : 0), "matrix if XBASIS");
    constexpr int TAU = F::TAU;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    typename F::word v[TAU];
#pragma unroll
    for (int q = 0; q < TAU; q++) v[q] = soa[(size_t)q * n + i];
    if constexpr (XBASIS) {
        const typename F::XbMat &M = opt_arg<typename F::XbMat>(opt...);
#pragma unroll 1
        for (int r = 0; r < TAU; r++) {
            typename F::word s = F::mul(M.m[TAU * r], v[0]);
#pragma unroll
            for (int q = 1; q < TAU; q++) s = F::add(s, F::mul(M.m[TAU * r + q], v[q]));
            aos[i * TAU + r] = F::to_canon(s);
        }
    } else {
#pragma unroll
        for (int q = 0; q < TAU; q++) aos[i * TAU + q] = F::to_canon(v[q]);
    }
}
template <class F>
void launch_ext_to_aos(const typename F::word *soa, u64 *aos, size_t n, hipStream_t s, const typename F::XbMat *T) {
    if (!n) return;
    const dim3 g(cdiv(n, 256)), b(256);
    if (T) hipLaunchKernelGGL((k_ext_to_aos<F, true>), g, b, 0, s, soa, aos, n, *T);
    else hipLaunchKernelGGL((k_ext_to_aos<F, false>), g, b, 0, s, soa, aos, n);
}
// A ring table [RE][n] that must be slot-constant (the eq tables of lf_sumcheck_fold_begin_dev, which the host cannot inspect): bit 1 of *flag goes up where
// slot k > 0 of an entry differs from slot 0.  (Equal field elements are equal device words on both rings.)
template <class F>
__global__ void __launch_bounds__(256) k_slot_const_check(const typename F::word *tab, size_t n, u32 *flag) {
    constexpr int RE = F::RE, TAU = F::TAU;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, st = (size_t)gridDim.x * 256;
    bool bad = false;
    for (; idx < (size_t)(RE - TAU) * n; idx += st) {
        const size_t w = TAU + idx / n, i = idx % n;
        bad |= tab[w * n + i] != tab[(w % TAU) * n + i];
    }
    if (bad) atomicOr(flag, 2u);
}
template <class F>
void launch_slot_const_check(const typename F::word *tab, size_t n, u32 *flag, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_slot_const_check<F>, dim3(grid_for((size_t)(F::RE - F::TAU) * n)), dim3(256), 0, s, tab, n, flag);
}

// rows [row0, row0 + kappa) of the synthetic Ajtai matrix into A [kappa][RE][n]: columns [col0, col0 + n) of the n_total-column matrix
template <class F>
__global__ void __launch_bounds__(256) k_fill_ajtai(typename F::word *A, u32 kappa, size_t n, size_t n_total, size_t col0, u64 seed, u32 row0) {
    constexpr int RE = F::RE;
    size_t total = (size_t)kappa * RE * n;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, st = (size_t)gridDim.x * 256;
    for (; i < total; i += st) {
        size_t j = i % n, w = (i / n) % RE, row = row0 + i / (RE * n);
        A[i] = F::from_canon(F::splitmix(seed, (row * n_total + col0 + j) * RE + w));
    }
}
template <class F>
void launch_fill_ajtai(typename F::word *A, u32 kappa, size_t n, size_t n_total, size_t col0, u64 seed, hipStream_t s, u32 row0) {
    hipLaunchKernelGGL(k_fill_ajtai<F>, dim3(4096), dim3(256), 0, s, A, kappa, n, n_total, col0, seed, row0);
}

// ---------------------------------------------------------------------------------------------------------
// CRT: the three radix-2 layers over Y^8 - Y^4 + 1 = (Y^4 - w^4)(Y^4 - w^20) that evaluate one residue class of the coefficients at the 8 primitive 24th
// roots (stark-rings CRT; call sites arith.rs:238,327).  Tab: the ring's table struct (w4 .. w11).  The monomial twists behind them are the ring's (crt_store).
template <class F, class Tab>
__device__ __forceinline__ void crt8(const typename F::word x[8], typename F::word o[8], const Tab &t) {
    typedef typename F::word W;
    W lo[4], hi[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        W tt = F::mul(t.w4, x[i + 4]);
        lo[i] = F::add(x[i], tt);
        hi[i] = F::sub(F::add(x[i], x[i + 4]), tt);
    }
    W l0[2], l1[2], h0[2], h1[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        W tt = F::mul(t.w2, lo[i + 2]);
        l0[i] = F::add(lo[i], tt); l1[i] = F::sub(lo[i], tt);
        W uu = F::mul(t.w10, hi[i + 2]);
        h0[i] = F::add(hi[i], uu); h1[i] = F::sub(hi[i], uu);
    }
    W a = F::mul(t.w1, l0[1]);  o[0] = F::add(l0[0], a); o[1] = F::sub(l0[0], a);
    W b = F::mul(t.w7, l1[1]);  o[2] = F::add(l1[0], b); o[3] = F::sub(l1[0], b);
    W c = F::mul(t.w5, h0[1]);  o[4] = F::add(h0[0], c); o[5] = F::sub(h0[0], c);
    W d = F::mul(t.w11, h1[1]); o[6] = F::add(h1[0], d); o[7] = F::sub(h1[0], d);
}
// coefficient table [RE][n] -> NTT table [RE][n]; crt_store is the ring's own (found through Tab's namespace)
template <class F, class Tab>
__global__ void __launch_bounds__(256) k_crt_fwd(Tab t, const typename F::word *coef, typename F::word *ntt, size_t n) {
    constexpr int RE = F::RE;
    size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    typename F::word a[RE];
#pragma unroll
    for (int c = 0; c < RE; c++) a[c] = coef[(size_t)c * n + j];
    crt_store(a, ntt, n, j, t);
}
template <class F, class Tab>
void launch_crt_fwd(const Tab &t, const typename F::word *coef, typename F::word *ntt, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL((k_crt_fwd<F, Tab>), dim3(cdiv(n, 256)), dim3(256), 0, s, t, coef, ntt, n);
}

// ---------------------------------------------------------------------------------------------------------
// balanced decomposition on coefficient tables, power-of-two base (stark_rings::balanced_decomposition; call sites arith.rs:235,
// decomposition/utils.rs:23-31,48).  Sign-magnitude, |digit| <= base/2, ties kept.  (The digit loop is this kernel's own, not lfdec::DigitChain: see there
// for mode 1 at base 2^63.)
template <class F>
__global__ void __launch_bounds__(256) k_decompose(const typename F::word *coef, size_t n, u32 log_base, u32 digits, int layout, typename F::word *out, int mode) {
    constexpr int RE = F::RE;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * RE) return;
    size_t c = idx / n, i = idx % n;
    auto v = F::to_canon(coef[idx]);
    bool neg = v > (F::P - 1) / 2;
    u64 mag = neg ? F::P - v : v;
    u64 half = 1ULL << (log_base - 1), mask = (1ULL << log_base) - 1;
    size_t n_out = layout == 0 ? n * digits : n;
    int64_t cur = neg ? -(int64_t)mag : (int64_t)mag;   // |centred lift| <= (p-1)/2 < 2^63
    for (u32 k = 0; k < digits; k++) {
        int64_t dg;
        if (mode == 1 && log_base > 1) {
            // digit mode 1 (data, lf_set_digit_mode): floor / Euclidean rule, digits in [-base/2, base/2): rem = cur mod base, minus base if >= base/2
            int64_t rem = (int64_t)((u64)cur & mask);
            if ((u64)rem >= half) rem -= (int64_t)(mask + 1);
            cur = (cur - rem) >> log_base;
            dg = rem;
        } else {
            u64 rem = mag & mask;
            mag >>= log_base;
            if (rem > half) { dg = (int64_t)rem - (int64_t)(mask + 1); mag += 1; }
            else dg = (int64_t)rem;
            if (neg) dg = -dg;
        }
        size_t o = layout == 0 ? (c * n_out + i * digits + k) : ((size_t)k * RE * n + c * n + i);
        out[o] = F::from_i64(dg);
    }
}
template <class F>
void launch_decompose(const typename F::word *coef, size_t n, u64 base, u32 digits, int layout, typename F::word *out, hipStream_t s, int mode) {
    u32 lb = 0;
    while ((1ULL << lb) < base) lb++;
    if (n) hipLaunchKernelGGL(k_decompose<F>, dim3(cdiv(n * F::RE, 256)), dim3(256), 0, s, coef, n, lb, digits, layout, out, mode);
}
// out[i] = sum_j base^j in[i*digits + j] on any table (linear, either form)
template <class F>
__global__ void __launch_bounds__(256) k_recompose(const typename F::word *in, size_t n_out, typename F::word base, u32 digits, typename F::word *out) {
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_out * F::RE) return;
    size_t w = idx / n_out, i = idx % n_out;
    size_t n_in = n_out * digits;
    typename F::word acc = 0, pw = F::one();
    for (u32 j = 0; j < digits; j++) {
        acc = F::add(acc, F::mul(in[w * n_in + i * digits + j], pw));
        pw = F::mul(pw, base);
    }
    out[idx] = acc;
}
template <class F>
void launch_recompose(const typename F::word *in, size_t n_out, u64 base, u32 digits, typename F::word *out, hipStream_t s) {
    if (n_out) hipLaunchKernelGGL(k_recompose<F>, dim3(cdiv(n_out * F::RE, 256)), dim3(256), 0, s, in, n_out, F::from_canon(base % F::P), digits, out);
}
// coefficient table -> centred int32 planes; *viol: bit 0 if some |v| > bound, bit 2 if a value within the bound has no int32 (+2^31, possible only with
// B = 2^32, hence only where (p - 1) / 2 reaches it)
template <class F>
__global__ void __launch_bounds__(256) k_coef_to_i32(const typename F::word *coef, int32_t *planes, size_t total, u32 bound, int *viol) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, st = (size_t)gridDim.x * 256;
    int bad = 0;
    for (; i < total; i += st) {
        auto v = F::to_canon(coef[i]);
        bool neg = v > (F::P - 1) / 2;
        u64 mag = neg ? F::P - v : v;
        if (mag > bound) { bad |= 1; mag = 0; }
        if constexpr ((F::P - 1) / 2 > 0x7fffffffull) {
            if (!neg && mag > 0x7fffffffull) { bad |= 2; mag = 0; }
        }
        planes[i] = neg ? (int32_t)(0u - (u32)mag) : (int32_t)mag;
    }
    if (bad) atomicOr(viol, bad);
}
template <class F>
void launch_coef_to_i32(const typename F::word *coef, int32_t *planes, size_t n, u32 bound, int *viol, hipStream_t s) {
    hipLaunchKernelGGL(k_coef_to_i32<F>, dim3(grid_for(n * F::RE, 4096)), dim3(256), 0, s, coef, planes, n * F::RE, bound, viol);
}
template <class F>
__global__ void __launch_bounds__(256) k_i32_to_coef(const int32_t *planes, typename F::word *coef, size_t total) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, st = (size_t)gridDim.x * 256;
    for (; i < total; i += st) coef[i] = F::from_i64(planes[i]);
}
template <class F>
void launch_i32_to_coef(const int32_t *planes, typename F::word *coef, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_i32_to_coef<F>, dim3(grid_for(n * F::RE, 4096)), dim3(256), 0, s, planes, coef, n * F::RE);
}
// l-infinity norm: max |centred coefficient| of a coefficient table -> *out_max
template <class F>
__global__ void __launch_bounds__(256) k_linf(const typename F::word *coef, size_t total, unsigned long long *out_max) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, st = (size_t)gridDim.x * 256;
    u64 mx = 0;
    for (; i < total; i += st) {
        auto v = F::to_canon(coef[i]);
        u64 mag = v > (F::P - 1) / 2 ? F::P - v : v;
        mx = mag > mx ? mag : mx;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        u64 o = __shfl_down((unsigned long long)mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out_max, (unsigned long long)mx);
}
template <class F>
void launch_linf(const typename F::word *coef, size_t n, u64 *out_max, hipStream_t s) {
    (void)hipMemsetAsync(out_max, 0, 8, s);
    hipLaunchKernelGGL(k_linf<F>, dim3(grid_for(n * F::RE, 4096)), dim3(256), 0, s, coef, n * F::RE, (unsigned long long *)out_max);
}

// ---------------------------------------------------------------------------------------------------------
// compute_f_0 (folding.rs:258-268) in the coefficient domain: f_0[j] = sum_i rho_i * f_i[j] mod the ring's cyclotomic polynomial of degree D exactly, with rho_i
// a short challenge (24 coefficients in [-32,32)) and f_i the bit-planes -> plain int32 convolutions.
// Nibble tables.  For one side, sum_k rho_k[a] * digit_k(v_c) = sign(v_c) * sum_nibbles R[nibble][value][a] with
// R[q][val][a] = sum_{b<4} bit_b(val) rho_{4q+b}[a]: NQ look-ups of a 24-vector and 24 additions per coefficient c replace the
// 4 NQ x 24 multiply-adds over the bit-planes.  The tables (both signs, both sides: 2*2*NQ*16*24 int32, 24 KB at NQ = 4) are built in LDS per block.
// Sliding window: coefficient c only touches positions c..c+23, so with both sides handled per group of 8 coefficients the positions
// C0..C0+7 are final after the group; they are stored (before the wrap of positions >= D) and leave the registers -- 31 live accumulators, not D + 23.
template <int C0, int NQ>
__device__ __forceinline__ void fw_group8(int32_t (&win)[31], const int32_t *pL, const int32_t *pR, size_t n, size_t j,
                                          const int32_t (*R)[2][NQ][16][28], int32_t *out) {
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const int32_t *pl = side ? pR : pL;
        int32_t vv[8];
#pragma unroll
        for (int i = 0; i < 8; i++) vv[i] = pl[(size_t)(C0 + i) * n + j];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            int32_t v = vv[i];
            u32 mg = (u32)(v < 0 ? -v : v), sg = v < 0;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const int4 *t = (const int4 *)R[side][sg][q][(mg >> (4 * q)) & 15];
#pragma unroll
                for (int w = 0; w < 6; w++) {
                    int4 x = t[w];
                    win[i + 4 * w] += x.x; win[i + 4 * w + 1] += x.y; win[i + 4 * w + 2] += x.z; win[i + 4 * w + 3] += x.w;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[(size_t)(C0 + i) * n + j] = win[i];
#pragma unroll
    for (int i = 0; i < 23; i++) win[i] = win[i + 8];
#pragma unroll
    for (int i = 23; i < 31; i++) win[i] = 0;
}
template <int C0, int D, int NQ>   // the groups C0, C0 + 8, .. < D in turn
__device__ __forceinline__ void fw_groups(int32_t (&win)[31], const int32_t *pL, const int32_t *pR, size_t n, size_t j, const int32_t (*R)[2][NQ][16][28],
                                          int32_t *out) {
    if constexpr (C0 < D) {
        fw_group8<C0, NQ>(win, pL, pR, n, j, R, out);
        fw_groups<C0 + 8, D, NQ>(win, pL, pR, n, j, R, out);
    }
}
// the tables R [side][sign][nibble][value][a] of a block (rows padded to 28 words: bank spread); NQ: nibbles of |v|, 4 for K <= 16 bit-planes, 8 for K <= 32
template <int NQ>
__device__ __forceinline__ void fw_tables(int32_t (*R)[2][NQ][16][28], u32 K, const int8_t *rho) {
    for (u32 idx = threadIdx.x; idx < 2 * NQ * 16 * 24; idx += 256) {
        u32 a = idx % 24, val = (idx / 24) % 16, q = (idx / (24 * 16)) % NQ, side = idx / (24 * 16 * NQ);
        int sum = 0;
#pragma unroll
        for (u32 b = 0; b < 4; b++)
            if (4 * q + b < K && ((val >> b) & 1)) sum += rho[(size_t)(side * K + 4 * q + b) * 24 + a];
        R[side][0][q][val][a] = sum;
        R[side][1][q][val][a] = -sum;
    }
}
// The kernel itself stays with the ring: its last step, the wrap of positions >= D, differs (in registers on X^24 = X^12 - 1, on the stored values on
// X^72 = X^36 - 1), and as a call from a shared shell it changes the schedule of the whole kernel (Goldilocks, NQ = 4: 332 VGPRs instead of 120).

// ---------------------------------------------------------------------------------------------------------
// witness tables (lfhip_tables.h)
// Witness::get_fhat (arith.rs:273-297): the TAU tables f-hat_j of one witness from its centred int32 planes [RE][N], straight into the caller's layout --
// out [TAU][m][RE] canonical AoS words, entry i of table j = the ring element whose slot k is the base-field constant f_coeff[i][8 j + k] (word TAU k holds
// it, the other words of the slot are 0), entries N <= i < m zero.  A pure write stream: block = (64 entries, one table): the 8 x 64 coefficients come in
// as eight 256-byte runs into LDS, the 64 RE words leave as one run of consecutive u64, every word written once -- two words (16 bytes) per lane and store
// where `out` is 16-byte aligned (V2; RE is even, so a pair never straddles two entries), one word otherwise.  A negative coefficient c leaves as p - |c|
// (the u64 sum below wraps to it).  An external basis changes nothing here: its matrix keeps e_0 (column 0 = e_0, ExtBasis::set), and a constant slot is
// c e_0.
constexpr int FHAT_TILE = 64;
template <class F>
__device__ __forceinline__ u64 fhat_word(const int32_t (*cf)[FHAT_TILE + 1], int e, int w) {
    const int32_t c = cf[w / F::TAU][e];
    return w % F::TAU ? 0 : (u64)(int64_t)c + (c < 0 ? (u64)F::P : 0);
}
template <class F, bool V2>
__global__ void __launch_bounds__(256) k_fhat(const int32_t *planes, size_t N, size_t m, u64 *out) {
    constexpr int RE = F::RE, TAU = F::TAU;
    static_assert(RE == 8 * TAU && RE % 2 == 0 && 8 * FHAT_TILE == 2 * 256, "eight slots; pairs of words; two loads per thread");
    __shared__ int32_t cf[8][FHAT_TILE + 1];
    const size_t i0 = (size_t)blockIdx.x * FHAT_TILE, j = blockIdx.y;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int k = threadIdx.x / FHAT_TILE + 4 * h, i = threadIdx.x % FHAT_TILE;   // 256 threads = 4 planes x 64 entries, twice
        cf[k][i] = i0 + i < N ? planes[(8 * j + k) * N + i0 + i] : 0;
    }
    __syncthreads();
    u64 *dst = out + (j * m + i0) * RE;
    const size_t left = m - i0 < (size_t)FHAT_TILE ? m - i0 : (size_t)FHAT_TILE;   // entries of this tile
    if constexpr (V2) {
        for (int idx = 2 * threadIdx.x; idx < (int)left * RE; idx += 512) {
            const int e = idx / RE, w = idx % RE;
            *(ulonglong2 *)(dst + idx) = make_ulonglong2(fhat_word<F>(cf, e, w), fhat_word<F>(cf, e, w + 1));
        }
    } else {
        for (int idx = threadIdx.x; idx < (int)left * RE; idx += 256) dst[idx] = fhat_word<F>(cf, idx / RE, idx % RE);
    }
}
template <class F>
void launch_fhat(const int32_t *planes, size_t N, size_t m, u64 *out, hipStream_t s) {
    const dim3 g(cdiv(m, FHAT_TILE), F::TAU), b(256);
    if (((uintptr_t)out & 15) == 0) hipLaunchKernelGGL((k_fhat<F, true>), g, b, 0, s, planes, N, m, out);
    else hipLaunchKernelGGL((k_fhat<F, false>), g, b, 0, s, planes, N, m, out);
}
// z = x || 1 || w_ccs (arith.rs:399-409) as the plane table [RE][n] the SpMV launchers read: the head, entries [0, l] -- x from l staged elements of canonical
// AoS words, then the ring's one; the tail is written in place by launch_recompose_crt (or copied from the witness's own w_ccs planes)
template <class F>
__global__ void __launch_bounds__(256) k_z_head(const u64 *x, size_t l, typename F::word *z, size_t n) {
    constexpr int RE = F::RE, TAU = F::TAU;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (l + 1) * RE) return;
    const size_t w = idx / (l + 1), i = idx % (l + 1);
    z[w * n + i] = i < l ? F::from_canon(x[i * RE + w]) : (w % TAU ? typename F::word(0) : F::one());
}
template <class F>
void launch_z_head(const u64 *x, size_t l, typename F::word *z, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_z_head<F>, dim3(cdiv((l + 1) * F::RE, 256)), dim3(256), 0, s, x, l, z, n);
}
// [n][RE] canonical u64 -> [n][RE] device words, element-major: k_aos_to_soa with the ELEM store (flag, Ti as for launch_aos_to_soa)
template <class F>
void launch_aos_words(const u64 *aos, typename F::word *dst, size_t n, hipStream_t s, u32 *flag, const typename F::XbMat *Ti) {
    if (!n) return;
    const dim3 g(cdiv(n, 64)), b(256);
    if (flag && Ti) hipLaunchKernelGGL((k_aos_to_soa<F, true, true, true>), g, b, 0, s, aos, dst, n, flag, *Ti);
    else if (flag) hipLaunchKernelGGL((k_aos_to_soa<F, true, false, true>), g, b, 0, s, aos, dst, n, flag);
    else if (Ti) hipLaunchKernelGGL((k_aos_to_soa<F, false, true, true>), g, b, 0, s, aos, dst, n, *Ti);
    else hipLaunchKernelGGL((k_aos_to_soa<F, false, false, true>), g, b, 0, s, aos, dst, n);
}

}  // namespace lfk
