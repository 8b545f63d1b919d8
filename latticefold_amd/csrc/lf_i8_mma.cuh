// lf_i8_mma.cuh -- the small things every int8 matrix-core translation unit needs (gfx950 v_mfma_i32_16x16x64_i8): lf_ajtai_i8 / lf_ajtai_i8g (commitments),
// lf_sv_rounds / bb_sv_rounds (sumcheck rounds 1-3), lf_dot_i8 / bb_dot_i8 (u_s / eta inner products), lf_fold_i8 (compute_f_0), lf_zk_i8 (z_k build).
// A namespace of its own, so that lf and lfbb both pull it in with `using namespace i8mma`; everything is forced inline: a kernel that uses a helper
// compiles to the machine code of the spelled-out form.  The GEMM kernels themselves, their tile structs and their pipelines stay in their files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace i8mma {
typedef int v4i __attribute__((ext_vector_type(4)));   // one MFMA operand (16 int8) or one accumulator quad per lane
static inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
// v_perm_b32: selector values 0-3 = bytes of lo, 4-7 = bytes of hi, 12 = 0x00
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    return 0;
#endif
}
// Balanced base-256 digits d_u in [-128, 127] of a word, as the int8 bytes of the result: sum_u d_u 256^u = the word or, for a Goldilocks word, the word - p.
// With s = w + 0x80..80 the digits are byte_u(s) - 128, i.e. byte_u(s) ^ 0x80 as int8 -- no bias column in the GEMM.
__host__ __device__ __forceinline__ uint64_t balanced_bytes(uint64_t w) {   // a canonical Goldilocks word
    uint64_t s = w + 0x8080808080808080ull;
    if (s < w) s += 0xFFFFFFFFull;   // wrapped past 2^64: digits of w - p (2^64 - p = 2^32 - 1)
    return s ^ 0x8080808080808080ull;
}
__host__ __device__ __forceinline__ uint32_t balanced_bytes(uint32_t w) {   // a centred Montgomery word of BabyBear, |w| < 2^30: no wrap
    return (w + 0x80808080u) ^ 0x80808080u;
}
// One MFMA operand register from four 32-bit words: byte ub of w0, w1, w2, w3, in that order (three v_perm_b32)
constexpr uint32_t SEL_LO = 0x0C0C0400u, SEL_PAIR = 0x05040100u;   // byte 0 of the low source, byte 0 of the high source | two bytes of each
__device__ __forceinline__ uint32_t gather_bytes(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t ub) {
    const uint32_t sel = SEL_LO + ub * 0x0101u;   // bytes ub of both sources
    const uint32_t p01 = perm(w1, w0, sel), p23 = perm(w3, w2, sel);
    return perm(p23, p01, SEL_PAIR);
}
// Inner-dimension order of a K-step of 64 columns in the dot kernels: operand position 16 g + 2 t + h (lane group g, element e = 2 t + h of its 16) holds
// column 8 t + 2 g + h -- so that ONE load instruction (16 bytes per lane) reads 64 contiguous bytes per vector row (the four lane groups of a row side by
// side) instead of 16 bytes from each of 64 different cache lines.  The X loads take kstep_col(first column, g, e); the packed Y digits are stored by position.
template <class T>
__host__ __device__ __forceinline__ constexpr T kstep_col(T base, uint32_t g, uint32_t e) { return base + 8 * (e >> 1) + 2 * g + (e & 1); }
__host__ __device__ __forceinline__ constexpr uint32_t kstep_col(uint32_t pos) { return 8 * ((pos & 15) >> 1) + 2 * (pos >> 4) + (pos & 1); }
}  // namespace i8mma
