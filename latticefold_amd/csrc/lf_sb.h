// lf_sb.h -- the small-base path of the Goldilocks prover: decomposition bases b = 4, 8, 16 (DecompositionParams::B_SMALL,
// decomposition_parameters.rs:17).  At b = 2 the K parts of a witness are virtual bit planes of its int32 coefficient planes; for b > 2 they are
// materialised once per decomposition as digit planes
//     D : uint8 [K][24][ldn],  byte = 64 + digit_k(coefficient),  ldn = 8 ceil(N / 8),  columns past N hold 64 (digit 0)
// -- the operand words of the general int8 commitment (lf_ajtai_i8g.hip: `pre`, 8 columns per 64-bit word), so the K - 1 part commitments read them in place.
// Every launcher returns 0, or -1 when the launch failed (the caller returns LF_ERR_HIP).
#pragma once
#include "lf_kernels.h"

namespace lf {

inline size_t sb_ld(size_t N) { return (N + 7) / 8 * 8; }
inline bool sb_base_ok(u32 b) { return b == 4 || b == 8 || b == 16; }
inline u32 sb_log2(u32 b) { u32 l = 0; while ((1u << l) < b) l++; return l; }

// largest magnitudes K balanced base-b digits reach under a digit rule (lf_set_digit_mode): mode 0 (sign-magnitude, ties kept) +-(b/2)(b^K - 1)/(b - 1);
// mode 1 (floor rule, digits in [-b/2, b/2)) only (b/2 - 1)(b^K - 1)/(b - 1) on the positive side.  A witness handle holds |coefficient| <= B/2 (the bound the
// ingest checks, whatever rule cut it): covered iff every such value has an exact K-digit form.
inline bool sb_digits_cover(u32 b, u32 K, u64 B, int mode) {
    if (b < 2 || (b & (b - 1)) || K == 0 || K > 64) return false;
    unsigned __int128 geo = 0, pw = 1;   // (b^K - 1) / (b - 1) = 1 + b + .. + b^(K-1)
    for (u32 k = 0; k < K; k++) { geo += pw; pw *= b; if (geo > ((unsigned __int128)1 << 80)) break; }
    const unsigned __int128 half = B / 2;
    if (b == 2) return geo >= half;      // bit planes of |v| with the sign: both rules
    if (mode == 0) return (unsigned __int128)(b / 2) * geo >= half;
    return (unsigned __int128)(b / 2 - 1) * geo >= half;
}

// the part cut: int32 coefficient planes [24][N] -> D (k_decompose's digit rule, lfdec::DigitChain)
int launch_sb_cut(const int32_t *planes, size_t N, u32 K, u32 lb, int mode, unsigned char *D, size_t ldn, hipStream_t s);
// z_k tails: out_k[off + i] = CRT( sum_l B^l * D[k][.][i L + l] ), out_k = out + k * 24 * ldz  (launch_recompose_crt on the digit planes; lf_kernels.hip)
int launch_sb_recompose_crt(const DevCrt &t, const unsigned char *D, size_t ldn, u32 wit_len, u32 L, u64 B, u32 K, u64 *out, size_t ldz, size_t off, hipStream_t s);
// v_s / theta: out[k][c][q] = sum_{i < n} eq[q][i] * digit(D[k][c][i]), canonical.  partial: sb_eval_partial_words(K) words
size_t sb_eval_partial_words(u32 K);
int launch_sb_eval(const unsigned char *D, size_t ldn, size_t n, const u64 *eq, size_t ldeq, u32 K, u64 *partial, u64 *out, hipStream_t s);
// G[row][slot] += sum_k sum_d apow[k][d] * digit(D[k][8d + slot][row]), rows < n
int launch_sb_add_fhat_comb(const unsigned char *D, size_t ldn, size_t n, u32 K, const Fq3Const *apow_dev, u64 *G, size_t m, hipStream_t s);
// the norm part of a round message of the folding sumcheck at degree 2b (nifs/folding/utils.rs:273-325):
//     out[X * 24 + 3 slot + q] = sum_p eqB(X, p) * sum_{k,d} mu_k^(d+1) * f (f^2 - 1) .. (f^2 - (b-1)^2),  f = fhat_kd(X, p),  X = 0 .. 2b
// F != null: the materialised tables F [2K*3][24][ldF]; else round 1 from the digit planes (f-hat virtual).  The G part (degree 2) comes from launch_fold_round_g.
// partial: sb_round_partial_words() words; out: sb_round_out_words() words
size_t sb_round_partial_words();
size_t sb_round_out_words();
int launch_sb_round(const DevCrt &t, u32 b, const FoldRoundArgs &a, const u64 *F, size_t ldF, const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n_planes,
                    u32 K, const Fq3Const *mu_pow_dev, u64 *partial, u64 *out, hipStream_t s);
// after r_1: F[2K*3][24][m/2], entry j = d(2j) + r1 (d(2j+1) - d(2j))
int launch_sb_materialize(const DevCrt &t, const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n_planes, size_t m, u32 K, Fq3Const r1, u64 *F, hipStream_t s);
// compute_f_0 in the coefficient domain: out[c][j] = (sum_i rho_i * part_i[j])(c) mod X^24 - X^12 + 1, rho_dev int8 [2K][24]
int launch_sb_fold_witness(const unsigned char *DL, const unsigned char *DR, size_t ldn, size_t n, u32 K, const int8_t *rho_dev, int32_t *out, hipStream_t s);

}  // namespace lf
