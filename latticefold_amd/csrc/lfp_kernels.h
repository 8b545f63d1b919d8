// lfp_kernels.h -- LatticeFold+ slice on the Frog ring Z_p[X]/(X^16 + 1), p = 15912092521325583641, COEFFICIENT form
// (the ring the reference runs latticefold-plus on: cyclotomic-rings/src/rings/frog.rs, crates/latticefold-plus/src/rgchk.rs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace lfp {
typedef uint64_t u64;
typedef uint32_t u32;
constexpr u64 P = 15912092521325583641ull;
constexpr int D = 16;
constexpr int TJ = 32;        // witness rows per LDS tile
constexpr int IG = 4;         // commitment-matrix rows per launch group
constexpr int KG = 4;         // digit planes per launch group
constexpr int RED_WAVES = 16;  // waves per block of the partial-sum reduction

struct Phase1Args {
    const u64 *f;       // n x 16 canonical words
    const u64 *A;       // kappa x n x 16
    u64 n;
    u32 kappa, i0, icnt;
    u32 k, k0, kcnt;
    u64 b;              // digit base
    int sh;             // log2(b) when b is a power of two, else -1
    u32 J;              // rows per block (multiple of TJ)
    int8_t *Df;         // [k][n][16], written when write_df
    u64 *part;          // [nblk][k*kappa*256 + kappa*16] partial sums mod p: comM_f coefficients, then A f
    u32 *err;
    int write_df, do_f;
};
struct Phase2Args {
    const u64 *A;
    const u64 *tau;     // n canonical words
    u64 n;
    u32 kappa, i0, icnt;
    u32 J;
    int8_t *mtau;       // n exponents (centred tau), written when i0 == 0
    u64 *part;          // [nblk][2*kappa*16] partial sums mod p: A tau, then A exp(tau)
    u32 *err;
};
void launch_phase1(const Phase1Args &a, u32 nblk, hipStream_t s);
void launch_phase2(const Phase2Args &a, u32 nblk, hipStream_t s);
void launch_mtau_all(const u64 *tau, u64 n, int8_t *mtau, u32 *err, hipStream_t s);
// out[o] = sum over blocks of part[blk][o] mod p; with l != 0 the first nsplit outputs (comM_f, [k][kappa][16][16]) are also cut into
// their l gadget digits: tau = split(hconcat(comM_f), n, base, l) (utils.rs:12-43), positions [0, kappa*k*16*l*16)
void launch_reduce(const u64 *part, u32 nblk, u32 nout, u64 *out, u32 nsplit, u32 kappa, u32 k, u64 base, u32 l, u64 *tau, hipStream_t s);
// ComR1CS::new (lfp_ingest.hip): f = z.gadget_decompose(b, k) and the block partial sums of A f for rows [i0, i0 + icnt) of A
struct IngestArgs {
    const u64 *z;       // m x 16 words (checked for canonicity when first: bit 4 of err)
    const u64 *A;       // kappa x n x 16
    u64 *f;             // n x 16 canonical words, written when first
    u64 m, n;           // n = m k
    u32 kappa, i0, icnt;
    u32 k;
    u64 b;
    int sh;             // log2(b) when b is a power of two, else -1
    u32 JZ;             // z elements per block (multiple of 16)
    u64 *part;          // [nblk][kappa*16] partial sums mod p
    u32 *err;
    int first;
};
hipError_t launch_ingest(const IngestArgs &a, u32 nblk, hipStream_t s);      // icnt in {1, 2, 4}; returns the launch's error
// the seeded commitment matrix (k_fill_ajtai): out[w] = splitmix64(seed + (w + 1) G) mod p for w < words (a multiple of 16; out 16-byte aligned)
hipError_t launch_fill_ajtai(u64 *out, u64 words, u64 seed, hipStream_t s);
// largest launch group (1, 2 or 4) not above `left`
inline u32 group_size(u32 left) { return left >= 4 ? 4 : left >= 2 ? 2 : 1; }
// Decomp::decompose (decomp.rs:32-99): base-B split, fix_variables over ring tables, sparse mat-vec with ring coefficients
void launch_decompose2(const u64 *f, size_t words, u64 B, u64 *F0, u64 *F1, hipStream_t s);
void launch_ring_fix(const u64 *in, u64 *out, u32 ntab, size_t len, const u64 *rM /* [2][16] Montgomery */, hipStream_t s, int const_r = 0);   // const_r: both coordinates are constant polynomials
void launch_spmv_ring(const u32 *rowptr, const u32 *col, const u64 *valM, const u64 *x, size_t nrows, u64 *y, hipStream_t s, int const_coef = 0);   // const_coef: every coefficient is a constant polynomial AND valM holds the constant terms alone, one word per non-zero (LfpMatrix::spmv_vals)
void launch_replicate(const u64 *src, size_t words, u32 copies, u64 *dst, hipStream_t s);
// ---- set check / range check (lfp_rgchk.hip; setchk.rs:65-262, rgchk.rs:81-186) ----------------------------------------------------------
constexpr int8_t LFP_ABSENT = -128;   // a zero entry of a monomial set (an absent sparse-matrix coefficient)
struct PwTab { u64 p[16], q[16]; };   // beta^t and beta^(2t), Montgomery
struct EqPt { u64 c[32], nc[32], one; };   // c_j, 1 - c_j and 1, Montgomery
struct ScDesc { u32 nmat, ncols, nvec, nsets_eff; };   // nsets_eff: sets entering the sumcheck polynomial (setchk.rs:160-197: all, or the first matrix set alone without a batching challenge)
void launch_sc_tables(const int8_t *dig, size_t n, u32 ncols, const PwTab &pw, u64 *tab, size_t ld, hipStream_t s);
void launch_eq_build(const EqPt &pt, u32 nv, u64 *eq, hipStream_t s);
u32 sc_round_max_blocks();
u32 launch_sc_round(const u64 *tab, size_t ld, size_t half, const ScDesc &d, const u64 *coef, u64 *part /* sc_round_max_blocks * 4; returns the blocks used */, hipStream_t s);
void launch_sc_fix(const u64 *in, u64 *out, size_t ld, u32 ntab, size_t half, u64 rM, hipStream_t s);
// the same round / fix + round from the exponent digits of ONE set (ncols 16 or 1; returns the blocks used, 0 = shape not handled): no beta^e tables exist
u32 launch_sc_round0_dig(const int8_t *dig, size_t n, u32 ncols, const PwTab &pw, const u64 *eq, const u64 *coef, u64 *part, hipStream_t s);
u32 launch_sc_fix_round_dig(const int8_t *dig, size_t n, u32 ncols, const PwTab &pw, const u64 *eq, u64 rM, u64 *tab /* the set's 2 ncols + 1 tables */, size_t ld,
                            const u64 *coef, u64 *part, hipStream_t s);
u32 eval_chunks(size_t n);
void launch_sum_parts(const u64 *part, u32 chunks, size_t stride, u32 nout, u64 *out, hipStream_t s);      // out[o] = sum_chunk part[chunk * stride + o]
// out[col][16] = sum_row w[row] X^e(dig[row][col]); wstride 1: scalar Montgomery weights (out canonical), 16: canonical ring weights.  part: eval_chunks(n) * ncols * 16
void launch_wmono(const int8_t *dig, size_t n, u32 ncols, const u64 *w, u32 wstride, u64 *part, u64 *out, hipStream_t s);
// 16 columns against nw <= 4 SCALAR weight tables (Montgomery) in one pass (exponent histogram): out[q * ostride + col * 16 + t]; part: nw * eval_chunks(n) * 256 words
void launch_whist16(const int8_t *dig, size_t n, const u64 *const *w, u32 nw, u64 *part, u64 *out, size_t ostride, hipStream_t s);
// out[16] = sum_row w[row] f[row]; part: eval_chunks(n) * 16
void launch_wring(const u64 *f, size_t n, const u64 *w, u32 wstride, u64 *part, u64 *out, hipStream_t s);
// out[0] = sum_i x[i xstride] y[i]; part: eval_chunks(n) * 4
void launch_wdot(const u64 *x, u32 xstride, int x_mont, const u64 *y, size_t n, u64 *part, u64 *out, hipStream_t s);
void launch_spmvT_eq(const u32 *colptr, const u32 *rowidx, const u64 *val, const u64 *eq, size_t n, u64 *w, hipStream_t s);
void launch_spmvT_eq_const(const u32 *colptr, const u32 *rowidx, const u64 *val, const u64 *eq, size_t n, u64 *w, hipStream_t s);   // scalar w (Montgomery): constant-coefficient M
// ---- Cm::prove (cm.rs:56-347)
struct CmShort { int32_t v[3][16]; };     // the three folding challenges s (centred coefficients)
struct CmDesc { u32 L, nM; };
void launch_cm_materialize(const int8_t *dig, const u64 *tau, size_t n, u64 *out, hipStream_t s);
// compact instance tables of Cm::prove: m_tau as exponent bytes, M_q tau as scalars (lfp_rgchk.hip)
struct CmCompact { const int8_t *mtau[8]; const u64 *mts; size_t ldm; };      // mts[(l nM + q) ldm + row], canonical
struct CmTabList { uint16_t idx[64]; };
void launch_spmv_scalar_const(const u32 *rowptr, const u32 *col, const u64 *valM, const u64 *x, size_t nrows, u64 *y, hipStream_t s);
void launch_spmv_mono_const(const u32 *rowptr, const u32 *col, const u64 *valM, const int8_t *dig, size_t nrows, u64 *y, hipStream_t s);
void launch_to_mont(const u64 *in, size_t n, u64 *out, hipStream_t s);
void launch_cm_h(const int8_t *Df, size_t n, u32 k, const int32_t *sp, u64 *h, hipStream_t s);
void launch_cm_g(const u64 *tau, const int8_t *mtau, const u64 *f, const u64 *h, size_t n, const CmShort &s, u64 *g, hipStream_t st);
// the round with fix_variables of the previous round fused in (S / R: the previous tables, 4 entries per new pair; the fixed tables go to So / Ro, ld_o entries per table)
void launch_cm_round_fused(const u64 *S, size_t lds, const u64 *R, size_t ldr, size_t half, const CmDesc &d, const u64 *rcp, u64 rM, u64 *So, u64 *Ro, size_t ld_o, u64 *part,
                           hipStream_t s);
u32 cm_round_blocks(size_t half);
void launch_cm_round(const u64 *S, size_t lds, const u64 *R, size_t ldr, size_t half, const CmDesc &d, const u64 *rcp, u64 *part /* blocks * 48 */, hipStream_t s);
void launch_cm_fix(const u64 *in, size_t ld_in, u64 *out, size_t ld_out, u32 w, u32 ntab, size_t half, u64 rM, hipStream_t s);
// the sumcheckers through batched tables (S2 = eq | V, R2 = U | Z: lfp_rgchk.hip); evaluations of ring tables at the point of `eq` (part: cm_eval_chunks(n) * ntab * 16)
void launch_cm_combine(const u64 *S, size_t lds, const u64 *R, size_t ldr, size_t n, const CmDesc &d, const u64 *rcp, u64 *S2, u64 *R2, size_t ld2, hipStream_t s);
void launch_cm2_round(const u64 *S, size_t lds, const u64 *R, size_t ldr, size_t half, u64 *part /* blocks * 48 */, hipStream_t s);
void launch_cm2_round_fused(const u64 *S, size_t lds, const u64 *R, size_t ldr, size_t half, u64 rM, u64 *So, u64 *Ro, size_t ld_o, u64 *part, hipStream_t s);
u32 cm_eval_chunks(size_t n);
void launch_cm_evals(const u64 *R, size_t ldr, size_t n, const u64 *eq, u32 ntab, u64 *part, u64 *out, hipStream_t s);
void launch_cm_combine_c(const u64 *S, size_t lds, const u64 *R, size_t ldr, size_t n, const CmDesc &d, const u64 *rcp, const CmCompact &cc, u64 *S2, u64 *R2, size_t ld2, hipStream_t s);
void launch_cm_evals_c(const u64 *R, size_t ldr, size_t n, const u64 *eq, u32 ntab, const CmTabList &dense, u32 ndense, const CmCompact &cc, u32 L, u32 nM, u32 per, u64 *part,
                       u64 *out, hipStream_t s);
// ---- ComR1CS::linearize (r1cs.rs:76-139): degree-3 round of eq (ga gb - gc); part: cm_round_blocks(half) * 64
void launch_r1cs_round_fused(const u64 *E, const u64 *G, size_t ld, size_t half, u64 rM, u64 *Eo, u64 *Go, size_t ld_o, u64 *part, hipStream_t s);   // + fix_variables of the previous round (E / G: previous tables)
void launch_r1cs_round(const u64 *E, const u64 *G, size_t ld, size_t half, u64 *part, hipStream_t s);
// ---- linearization of a committed CCS instance (lfp_ccs.hip; lfplus_ccs_linearize): one round of eq * sum_i c_i prod_{j in S_i} g_j at the points 0 .. d + 1.
// The shape, as the host classified it once (lfp_ccs.h): chain i multiplies the tables op[i][0 .. len[i]); its coefficient is CCS_ZERO (lev[i] = 0: the chain is
// skipped), CCS_ONE / CCS_MINUS_ONE, CCS_CONST (a base-field constant, cst[i] in Montgomery form: a word-wise multiply) or CCS_GENERAL (one more negacyclic product,
// against coefficient i of `coef`).  lev[i] = len[i] + (general ? 1 : 0) operands enter chain i, so it costs lev[i] - 1 negacyclic products; maxlev = max_i lev[i];
// slot[i]: the LDS slot of the running product of a chain with lev[i] >= 2 (nslots of them)
enum { CCS_ZERO = 0, CCS_ONE = 1, CCS_MINUS_ONE = 2, CCS_CONST = 3, CCS_GENERAL = 4 };
struct CcsDesc {
    u32 t, q, maxlev, nslots;
    uint8_t len[8], lev[8], cls[8], slot[8];
    uint8_t op[8][8];
    u64 cst[8];
};
u32 ccs_round_blocks(size_t half, u32 cap);      // workgroups of a round over `half` pairs: 16 pairs each and pass, at most cap
// E: eq(r, .) as Montgomery scalars, ONE word per row; G: the t tables g_j, canonical, [table][ld][16]; coef: q x 16 canonical words (device); np = d + 2 points
// (3 .. 9).  part[block][np][16] canonical block partials.  The fused form reads the PREVIOUS tables (4 entries per new pair), fixes them at rM (Montgomery) on
// the way in and stores the fixed tables to Eo / Go (ld_o entries per table)
void launch_ccs_round(const u64 *E, const u64 *G, size_t ld, size_t half, const CcsDesc &d, u32 np, const u64 *coef, u32 blocks, u64 *part, hipStream_t s);
void launch_ccs_round_fused(const u64 *E, const u64 *G, size_t ld, size_t half, const CcsDesc &d, u32 np, const u64 *coef, u64 rM, u64 *Eo, u64 *Go, size_t ld_o, u32 blocks,
                            u64 *part, hipStream_t s);
// *first_bad = min(*first_bad, smallest row r < nrows with sum_i c_i prod_{j in S_i} (M_j f)[r] != 0) (lfp_check.hip); vals / const_coef as launch_r1cs_residual,
// coefM: q x 16 MONTGOMERY words (device)
void launch_ccs_residual(const u32 *const *rowptr, const u32 *const *col, const u64 *const *vals, const int *const_coef, const CcsDesc &d, const u64 *coefM, const u64 *f,
                         size_t nrows, u64 *first_bad, hipStream_t s);
// ---- the generic sumcheck (lfp_mlsumcheck.hip; lfplus_mlsumcheck_*): g = sum_i coef_i prod_{k in [off[i], off[i + 1])} T_{idx[k]} over nt ring tables [table][ld][16]
struct MlsDesc {
    u32 nt, nterms, degree;
    uint8_t off[17], idx[64];
    uint8_t cls[16];          // the coefficient of term i: MLS_ZERO (the term is skipped), MLS_ONE / MLS_MINUS_ONE (the constants: no coefficient product), MLS_GENERAL
};
enum { MLS_ZERO = 0, MLS_ONE = 1, MLS_MINUS_ONE = 2, MLS_GENERAL = 3 };
u32 mls_round_blocks(size_t half, u32 cap);      // workgroups of a round over `half` pairs: 16 pairs each and pass, at most cap
// one round: part[block][degree + 1][16] canonical block partials of the evaluations at 0 .. degree.  coef: nterms x 16 canonical words (device).  The fused form
// reads the PREVIOUS tables (4 entries per new pair), fixes them at rM (Montgomery) on the way in and stores the fixed tables to out (ld_out entries per table)
void launch_mls_round(const u64 *in, size_t ld_in, size_t half, const MlsDesc &d, const u64 *coef, u32 blocks, u64 *part, hipStream_t s);
void launch_mls_round_fused(const u64 *in, size_t ld_in, size_t half, const MlsDesc &d, const u64 *coef, u64 rM, u64 *out, size_t ld_out, u32 blocks, u64 *part, hipStream_t s);
// out[t][16] = in[t][0] + r (in[t][1] - in[t][0]) for t < nt: the last variable of every table
void launch_mls_final(const u64 *in, size_t ld_in, u32 nt, u64 rM, u64 *out, hipStream_t s);
// ---- ring arithmetic on arrays (lfp_ring_ops.hip; lfplus_ring_mul): out[x] = sum_{i < n_terms} a_i[x] * b_i[x] for x < count, table i of a at a + i count 16.
// mode 0: b is n_terms x count canonical ring elements; mode 1: b is n_terms x 16 MONTGOMERY words (device), one coefficient per term.  n_terms <= 64.  a, out
// (and b in mode 0) are 16-byte aligned; out may be exactly a (or b in mode 0) when n_terms == 1 and overlaps nothing otherwise.  *flag |= 1 if a word of a
// (of b in mode 0) is not canonical.  blocks = ring_mul_blocks(count, cap): one workgroup per 16 elements, at most cap
u32 ring_mul_blocks(u64 count, u32 cap);
void launch_ring_mul(const u64 *a, const u64 *b, u32 n_terms, u64 count, int mode, u64 *out, u32 *flag, u32 blocks, hipStream_t s);
// ---- MLE tables on arrays (lfp_tables.hip; lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t).  Tables are [table][len][16]
// canonical words, 16-byte aligned; a point is its coordinates in Montgomery form (host-converted) and travels as a kernel argument
struct TabPoint { u64 rM[28]; u64 oneM; };      // r_i 2^64 mod p for i < nv, and 2^64 mod p
constexpr u32 TAB_LO = 10;         // k_tab_eval: the eq weights of the low min(nv, 10) variables live in LDS; a workgroup takes 2^TAB_LO entries (a chunk) per pass
constexpr u32 TAB_FIX = 6;         // k_tab_fix: variables one launch fixes at most (each thread sums 2^6 entries)
constexpr u32 SPT_HEAVY = 64;      // k_spmv_t: a column of MORE entries is summed by the whole workgroup, 16 entries abreast
constexpr u32 SPT_FLUSH = 64;      // k_spmv_t: products of one 16-lane group before its lazy sum is reduced (the heavy path: a column of more than 16 * 64 entries)
// out[x] = (eq(point, x), 0, .., 0) for x < 2^nv
void launch_tab_eq(const TabPoint &pt, u32 nv, u64 *out, u32 cap, hipStream_t s);
u32 tab_eval_blocks(u64 len, u32 nv, u32 ntables, u32 cap);      // workgroups per table: one per chunk, at most max(1, cap / ntables)
// part[table][block][16] = the block's share of sum_{x < len} eq(point, x) T[x]; then out[table][16] = the sum over the blocks.  *flag |= 1: a word >= p
void launch_tab_eval(const u64 *tables, u32 ntables, u64 len, const TabPoint &pt, u32 nv, u32 blocks, u64 *part, u64 *out, u32 *flag, hipStream_t s);
// out[table][y] = sum_{t < 2^nf} eq(point[0 .. nf), t) in[table][y 2^nf + t] for y < nout, nf <= TAB_FIX; tables of `in` are ld_in entries apart, of out nout
void launch_tab_fix(const u64 *in, u64 ld_in, u32 ntables, u64 nout, const TabPoint &pt, u32 nf, u64 *out, u32 *flag, hipStream_t s);
// out[c] = sum over the entries k in [colptr[c], colptr[c + 1]) of val[k] * v[rowidx[k]] (negacyclic; val and v canonical) for c < n
void launch_spmv_t(const u32 *colptr, const u32 *rowidx, const u64 *val, const u64 *v, u64 n, u64 *out, hipStream_t s);
// ---- relation checks (lfp_check.hip): R_ComR1CS (r1cs.rs:21-60), R_LinB (lin.rs:29-40)
// *first_bad = min(*first_bad, smallest row r < nrows with ((M_0 f) (M_1 f) - M_2 f)[r] != 0); vals[q]: LfpMatrix::spmv_vals() of matrix q (const_coef[q] as there)
void launch_r1cs_residual(const u32 *const *rowptr, const u32 *const *col, const u64 *const *vals, const int *const_coef, const u64 *f, size_t nrows, u64 *first_bad,
                          hipStream_t s);
// out[q][16] = sum_row w[q ldw + row] f[row] for q < nw, nw in {2, 4, 8} (w: SCALAR weights, Montgomery; out canonical) in one pass over f; absmax (may be null):
// *absmax = max(*absmax, largest |centred word| of f).  part: eval_chunks(n) * nw * 16 words
void launch_linb_dots(const u64 *f, size_t n, const u64 *w, size_t ldw, u32 nw, u64 *part, u64 *out, u64 *absmax, hipStream_t s);
// *absmax = max(*absmax, largest |centred word| of x); flag (may be null): *flag |= 1 if a word is not canonical (lfp_digits.hip: the relation checks and lfplus_linf_norm)
void launch_absmax(const u64 *x, size_t words, u64 *absmax, hipStream_t s, u32 *flag = nullptr);
// ---- gadget maps on arrays (lfp_digits.hip; lfplus_balanced_decompose / _recompose, lfplus_set_matrices_gadget).  Arrays are [element][16] canonical words; digit i
// of element j sits at element j k + i (layout 0: gadget order) or i count + j (layout 1: planes).  blocks = digit_blocks(words, cap): 256 words each and pass
struct DigitPows { u64 pM[64]; };      // b^i 2^64 mod p for i < k
u32 digit_blocks(u64 words, u32 cap);
// out: the k balanced base-b digits (digit_step) of every centred word of in; *flag |= 1: a word >= p
void launch_digits_decompose(const u64 *in, u64 count, u64 b, u32 k, int layout, u64 *out, u32 *flag, u32 blocks, hipStream_t s);
// out[j] = sum_{i < k} b^i in[digit i of j], word by word mod p (in: general canonical words); *flag |= 1: a word >= p
void launch_digits_recompose(const u64 *in, u64 count, u32 k, int layout, const DigitPows &pw, u64 *out, u32 *flag, u32 blocks, hipStream_t s);
// The gadget form of a short CSR matrix (rows x m, nnz entries e with ring coefficients val[e][16], canonical) as a complete n x n LfpMatrix, n = m k: entry e at
// (r, j) becomes the k entries e k + i at (r, j k + i) with val b^i.  rowptr_s has rows + 1 entries, colptr_s (the short column pointers) m + 1.
// perm[pos] = the CSR index of the entry at position pos of the short CSC order (column-major, rows ascending): launch_gadget_perm, a stable sort of the entries by
// column (tmp: gadget_perm_bytes(nnz, m) bytes)
size_t gadget_perm_bytes(u64 nnz, u64 m);
hipError_t launch_gadget_perm(const u32 *col_s, u64 nnz, u64 m, u32 *perm, void *tmp, size_t tmp_bytes, hipStream_t s);
struct GadgetOut { u32 *rowptr, *col, *colptr, *rowidx; u64 *valM, *valT, *valMc, *valTc; };      // valMc / valTc null: not a constant-coefficient matrix
void launch_gadget_expand(const u32 *rowptr_s, const u32 *col_s, const u64 *val_s, const u32 *colptr_s, const u32 *perm, u64 rows, u64 m, u64 n, u64 nnz, u32 k,
                          const DigitPows &pw, const GadgetOut &o, hipStream_t s);
void launch_vec_add(u64 *acc, const u64 *x, size_t n, hipStream_t s);
void launch_check_canonical(const u64 *x /* 16-byte aligned */, size_t n, u32 *flag, u32 bit, hipStream_t s);
// dst = src (`words` words, a multiple of 16; both 16-byte aligned, not overlapping) and *flag |= bit if a word is not canonical: one pass (k_copy_checked)
void launch_copy_checked(const u64 *src, u64 *dst, size_t words, u32 *flag, u32 bit, hipStream_t s);
void launch_tensor_level(const u64 *cur, u64 len, u64 r, u64 *nxt, hipStream_t s);
void launch_tensor_product(const u64 *a, u64 m, const u64 *b, u64 n, u64 *out, hipStream_t s);
}  // namespace lfp
