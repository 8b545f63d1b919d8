/*
 * lfplus.h -- C ABI of the LatticeFold+ slice of liblfhip.so (MI355X / gfx950): the DOUBLE COMMITMENT of the range-check instance,
 * on the ring the reference runs latticefold-plus on (FrogRing RqPoly: Z_p[X]/(X^16 + 1), p = 15912092521325583641, COEFFICIENT form,
 * 16 canonical little-endian u64 words per ring element).  SURVEY.md section 8(f) row 4.
 *
 * Reference interfaces replaced (crates/latticefold-plus):
 *   RgInstance::from_f(f, &A, &DecompParameters{b,k,l})      src/rgchk.rs:260-331   (bench: benches/double_commitment.rs:53-82)
 *     cfs -> decompose_to_vec(b, k) -> D_f           rgchk.rs:263-284
 *     M_f = exp(D_f), comM_f = A * M_f               rgchk.rs:286-303
 *     tau = split(hconcat(comM_f), n, d/2, l)        rgchk.rs:304-306, utils.rs:12-43
 *     m_tau = exp(tau); cm_f, C_Mf, cm_mtau          rgchk.rs:308-320
 *   Matrix::try_mul_vec (Ajtai commitment, coefficient form)   stark-rings-linalg, call sites rgchk.rs:313-319
 *   Decomp::decompose(&A, B)                         src/decomp.rs:32-99
 *   utils::tensor / tensor_product                   src/utils.rs:45-83 (KATs utils.rs:118-131)
 *   PoseidonTranscript<RqPoly>, utils::short_challenge       src/transcript.rs:20-78, src/utils.rs:87-101
 *   In::set_check / Out::verify                      src/setchk.rs:65-262 / 266-340
 *   Rg::range_check / Dcom::verify                   src/rgchk.rs:81-186 / 193-258
 *   PlusProver::{init, prove} / PlusVerifier::{init, verify}   src/plus.rs:15-146   (lfplus_prover_*, lfplus_verify: the objects, below)
 *   MLSumcheck::{prove, verify}_as_subprotocol over any product list   latticefold/src/utils/sumcheck.rs:53-104   (lfplus_mlsumcheck_*, near the end of this file)
 *   RqPoly products and SparseMatrix x vector on arrays (the g_q = M_q f and g_A o g_B - g_C of r1cs.rs:76-95 as calls of their own)   (lfplus_ring_mul, lfplus_spmv, at the end of this file)
 *   DenseMultilinearExtension::{evaluate, fix_variables}, the eq(r, .) table and the transposed matrix product on arrays   (lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t, behind them)
 *
 * M_f and m_tau are matrices / vectors of unit monomials; they cross this boundary as their EXPONENT digits (int8 in (-d/2, d/2)):
 * exp(a) = X^a for a >= 0 and X^(d + a) for a < 0.  The Rust binding rebuilds Matrix<R> from them if a caller needs the dense form
 * (INTEGRATION.md); nothing on this path does.
 *
 * Everything runs on the GPU; there is no CPU fallback (LFPLUS_E_NO_DEVICE).  Parity status: bit-exact against oracle/lfp.c, which is
 * pinned to the reference only through the tensor KATs -- the digit / gadget conventions of the un-vendored stark-rings crate are
 * restated from call sites (see oracle/lfp.h).
 */
#ifndef LFPLUS_H
#define LFPLUS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LFPLUS_D 16
#define LFPLUS_P 15912092521325583641ULL

enum {
    LFPLUS_OK = 0,
    LFPLUS_E_ARG = -1,        /* null pointer, non-canonical word, shape mismatch, parameter outside the envelope */
    LFPLUS_E_NO_DEVICE = -2,  /* no HIP device: the library has no CPU path */
    LFPLUS_E_HIP = -3,
    LFPLUS_E_EXP_DOMAIN = -4, /* a digit of f or of tau is outside (-d/2, d/2): the reference's exp() returns None and from_f panics */
    LFPLUS_E_SMALL_N = -5,    /* kappa*k*d*l*d >= n: the reference's split() panics ("small n unsupported") */
    LFPLUS_E_REJECT = -6      /* a verifier rejected the proof (*stage says where) */
};
#define LFPLUS_ABSENT (-128)  /* exponent digit of a zero entry of a monomial set (an absent sparse-matrix coefficient) */

typedef struct lfplus_ctx lfplus_ctx;
int lfplus_ctx_create(int device, lfplus_ctx **out);
void lfplus_ctx_destroy(lfplus_ctx *ctx);
/* Scratch memory (tables of the protocol stages) is pooled per context and, when a context is destroyed, kept in a process-wide per-device cache for the next
 * contexts (a prover built per proof would otherwise pay hipMalloc for every table inside every prove).  Bounded per device: LFPLUS_CACHE_GB when set (0 = off),
 * otherwise min(32 GB, a quarter of the device's memory).  Every allocator of the library releases the cache and retries before it reports out-of-memory.
 * lfplus_scratch_trim frees what the cache holds on `device` (< 0: on every device); lfplus_scratch_bytes returns the bytes it holds there now.
 * No counterpart in the reference (the Rust allocator owns its Vecs). */
void lfplus_scratch_trim(int device);
size_t lfplus_scratch_bytes(int device);
const char *lfplus_last_error(const lfplus_ctx *ctx);

/* ---- multi-GPU: one prover column-sharded over `world` ranks, one GPU each (BASELINE configs[4]) ------------------------------------------
 * Rank g owns rows [g n / world, (g + 1) n / world) of every n-indexed object: its COLUMNS of the commitment matrix (lfplus_set_matrix then takes the
 * kappa x n / world slice), its rows of D_f, of the set-check / Cm / linearization tables and of the folded witness g.  Witnesses (lfplus_set_witness, the
 * F0 / F1 lfplus_decompose returns) are whole on every rank, as the host hands them over; tau and m_tau (a short non-zero prefix) are rebuilt whole.
 * Exchanged, each as "all-gather + sum mod p": the partial commitments (2 per double commitment, 1 per lfplus_commit / lfplus_decompose), the partial
 * sumcheck round messages of the first log2(n / world) rounds (then the tables are gathered, one entry per rank, and the last log2(world) rounds run
 * replicated), the partial evaluations; all-gathered whole: h (per instance, only with constraint matrices) and the folded witness.  Every rank runs the
 * identical transcript and returns the identical proof.  Call before lfplus_set_matrix; contexts that lfplus_share_matrix the matrix share the transport.
 * n / world must be a power of two >= 4 world.  lfplus_set_sharding: host transport, `cb` must all-gather `words` u64 from every rank into
 * recv_all[world * words] in rank order and return 0 (gloo in the tests).  lfplus_dist_init: an RCCL communicator owned by the library (one rank per GPU,
 * xGMI) from a 128-byte ncclUniqueId that rank 0 obtains with lfplus_dist_unique_id and the launcher distributes; RCCL is loaded with dlopen. */
typedef int (*lfplus_exchange_fn)(void *user, const uint64_t *send, uint64_t *recv_all, size_t words);
int lfplus_set_sharding(lfplus_ctx *ctx, int rank, int world, lfplus_exchange_fn cb, void *user);
int lfplus_dist_unique_id(uint8_t *id128);
int lfplus_dist_init(lfplus_ctx *ctx, int rank, int world, const uint8_t *id128);
/* exchange log of the context's transport: number of exchanges, summed and maximal host-side latency in microseconds (reset != 0 clears it) */
int lfplus_dist_stats(lfplus_ctx *ctx, uint64_t *n_exchanges, double *total_us, double *max_us, int reset);
/* u64 words this rank contributed to its exchanges (reset != 0 clears the counter) */
int lfplus_dist_stats_words(lfplus_ctx *ctx, uint64_t *words_sent, int reset);
/* TIMING MODEL, not a transport (as lf_set_sharding_model in lfhip.h): rank `rank` of `world` with no peers; zeros stand in for their words.  The "proofs" of such a
 * prover are meaningless; tools/shard_model.py --lfplus measures a rank's share of a sharded PlusProver::prove with it on a one-GPU box. */
int lfplus_set_sharding_model(lfplus_ctx *ctx, int rank, int world);

/* Ajtai matrix A (kappa x n ring elements, row-major, coefficient form); stays resident in HBM.  kappa <= 64.  In a sharded context: the rank's columns,
 * kappa x (n / world), and `n` is that local width. */
int lfplus_set_matrix(lfplus_ctx *ctx, const uint64_t *A, uint32_t kappa, uint64_t n);
/* The commitment matrix generated on the device from a seed instead of uploaded: word w of the row-major kappa x n x 16 matrix is
 * splitmix64(seed + (w + 1) G) mod p, G = 0x9E3779B97F4A7C15 (the indexable stream of PlusWorkload.ajtai_matrix; lf_ajtai_generate is the counterpart on the
 * LatticeFold side).  A pure write stream: no host generation, no upload.  Preconditions as lfplus_set_matrix: kappa <= 64, n <= 2^32, before the witness
 * (LFPLUS_E_ARG once the context holds one); a sharded context is refused (a rank uploads its columns).  The _timed form repeats the fill `iters` times between
 * two HIP events: average ms. */
int lfplus_matrix_generate(lfplus_ctx *ctx, uint64_t seed, uint32_t kappa, uint64_t n);
int lfplus_matrix_generate_timed(lfplus_ctx *ctx, uint64_t seed, uint32_t kappa, uint64_t n, uint32_t iters, double *ms_avg);
/* use the commitment matrix resident in `from` (same device) without copying it; the allocation is reference-counted and lives until its last holder
 * re-uploads or is destroyed */
int lfplus_share_matrix(lfplus_ctx *ctx, lfplus_ctx *from);
/* witness vector f (n ring elements); stays resident */
int lfplus_set_witness(lfplus_ctx *ctx, const uint64_t *f, uint64_t n);
/* ComR1CS::new (src/r1cs.rs:48-60) on the resident matrix A (kappa x n): z = m ring elements (host pointer, canonical words), n = m * k.
 * f = z.gadget_decompose(b, k) (element j -> its k balanced base-b digits, least significant first, at rows [j k, (j + 1) k)) becomes the
 * context's resident witness, exactly as after lfplus_set_witness(f); cm_f (kappa * 16 words, may be NULL) = A f.  Only z crosses PCIe (a k-th of f);
 * its words are checked on the device behind the upload (LFPLUS_E_ARG for a non-canonical one), the digits are cut and committed in one pass over A.
 * Envelope: matrix set, context not sharded (LFPLUS_E_ARG; a sharded prover uploads f with lfplus_set_witness), m * k == n <= 2^28, 1 <= k <= 16,
 * 2 <= b <= 2^31 (a digit fits an int32; larger bases stay on lfplus_set_witness + lfplus_commit).  A value that does not fit k digits loses its remainder,
 * as in the reference.  Waits for a pending lfplus_rg_from_f_async pass first.  After ANY error return the context has no resident witness. */
int lfplus_witness_from_z(lfplus_ctx *ctx, const uint64_t *z, uint64_t m, uint64_t b, uint32_t k, uint64_t *cm_f);
/* the same, then the pass alone `iters` times back to back, timed with HIP events on the library's stream (z resident): average ms */
int lfplus_witness_from_z_timed(lfplus_ctx *ctx, const uint64_t *z, uint64_t m, uint64_t b, uint32_t k, uint32_t iters, double *ms_avg);
/* Matrix::try_mul_vec on the RESIDENT witness (no upload): out = A f, kappa * 16 words.  Waits for a pending lfplus_rg_from_f_async pass first.  A sharded
 * context is refused with LFPLUS_E_ARG (lfplus_commit is the call that exchanges the ranks' partial sums). */
int lfplus_commit_resident(lfplus_ctx *ctx, uint64_t *out);

/* RgInstance::from_f on the resident (A, f).  b >= 2 (digits must land in (-8, 8): b <= 14), 1 <= k <= 16, 1 <= l <= 64.
 * Results stay on the device until lfplus_rg_read. */
int lfplus_rg_from_f(lfplus_ctx *ctx, uint64_t b, uint32_t k, uint32_t l);
/* The same pass enqueued on the context's second stream; returns at once.  from_f needs the witness, the matrix and the parameters only -- no challenge --
 * so a prover issues it as soon as the witness is resident and lets it run next to the linearization's latency-bound sumcheck rounds (Mlin::mlin calls
 * from_f after every linearization, mlin.rs:52-60; the order is not observable).  lfplus_rg_from_f / lfplus_mlin with the same parameters collect the result
 * and report the pass's errors; every other call that touches the witness or the from_f buffers waits for the pass first (lfplus_join_async does only that).
 * A sharded context ignores the hint.  LFPLUS_NO_ASYNC_FROM_F=1 in the environment turns the hint off. */
int lfplus_rg_from_f_async(lfplus_ctx *ctx, uint64_t b, uint32_t k, uint32_t l);
int lfplus_join_async(lfplus_ctx *ctx);
/* Any pointer may be NULL.  Df: k*n*16 int8 (D_f[k_i][n_i][d_i]); comMf: k*kappa*16*16 words (comM_f[k_i][row][column] ring elements);
 * tau: n words; mtau: n int8 (exponent digits of m_tau); cm_f / C_Mf / cm_mtau: kappa*16 words each. */
int lfplus_rg_read(lfplus_ctx *ctx, int8_t *Df, uint64_t *comMf, uint64_t *tau, int8_t *mtau, uint64_t *cm_f, uint64_t *C_Mf, uint64_t *cm_mtau);
/* the same computation `iters` times back to back, timed with HIP events on the library's stream (inputs resident): average ms */
int lfplus_rg_from_f_timed(lfplus_ctx *ctx, uint64_t b, uint32_t k, uint32_t l, uint32_t iters, double *ms_avg);

/* Decomp::decompose(&A, B) (src/decomp.rs:32-99; no transcript) on the resident (A, f), n a power of two:
 *   F = f.decompose_to_vec(B, 2).transpose() -> (F0, F1);  C_i = A F_i;
 *   v_i = [(mle(F_i)(r_a), mle(F_i)(r_b)), then per matrix M_j (mle(M_j F_i)(r_a), mle(M_j F_i)(r_b))]
 * r_a / r_b: log2(n) ring elements each (the components of Decomp::r); the nm matrices have n rows, CSR with ring-element coefficients
 * (val[j]: 16 words per non-zero).  Outputs (any may be NULL): F0, F1 n*16 words; C0, C1 kappa*16; v0, v1 (1+nm)*2*16. */
int lfplus_decompose(lfplus_ctx *ctx, uint64_t B, const uint64_t *r_a, const uint64_t *r_b, uint32_t nm, const uint32_t *const *rowptr,
                     const uint32_t *const *col, const uint64_t *const *val, uint64_t *F0, uint64_t *F1, uint64_t *C0, uint64_t *C1, uint64_t *v0,
                     uint64_t *v1);
/* The same, with the parts left on the device: F0 / F1 become the resident witnesses of dst0 / dst1 (contexts of the same device and width; `ctx` itself may be
 * one of them -- its witness, the folded g, is consumed first).  The accumulator of a folding prover (plus.rs:96-103: the two LinB of one prove are inputs of the
 * next) then never crosses PCIe: 2 x 134 MB down and up again per prove at 2^20 rows.  lfplus_get_witness reads a context's resident witness back. */
int lfplus_decompose_resident(lfplus_ctx *ctx, uint64_t B, const uint64_t *r_a, const uint64_t *r_b, uint32_t nm, const uint32_t *const *rowptr,
                              const uint32_t *const *col, const uint64_t *const *val, lfplus_ctx *dst0, lfplus_ctx *dst1, uint64_t *C0, uint64_t *C1,
                              uint64_t *v0, uint64_t *v1);
int lfplus_get_witness(lfplus_ctx *ctx, uint64_t *f_out /* n * 16 words */, uint64_t n);

/* ---- relation checks on the resident (A, f): "is this instance satisfied?" without moving the witness (134 MB at 2^20 rows) to the host.  The reference has no
 * check_relation for LatticeFold+; the relations are the ones its structs define and its tests assert piecewise (decomp.rs:157-215, r1cs.rs:211-233).
 * Every component is evaluated; *failed is the OR of the LFPLUS_REL_* bits of the failing ones; the return value is LFPLUS_OK, or LFPLUS_E_REJECT when *failed != 0.
 * *absmax (may be NULL) = the largest |centred coefficient| of f (centred: w if w <= (p - 1) / 2, else p - w); the norm rule is the balanced one, absmax < bound
 * (bound 0: not checked).  Read-only: neither the witness, the from_f buffers nor a transcript is touched; a pending lfplus_rg_from_f_async pass is waited for.
 * Arguments are validated as by lfplus_decompose (CSR shape, canonical words, n a power of two): LFPLUS_E_ARG, as for a context without matrix or witness, a
 * NULL `failed`, and a sharded context (a rank holds only its columns of A; as lfplus_witness_from_z).  The context stays usable after every return. */
enum { LFPLUS_REL_CM = 1, LFPLUS_REL_R1CS = 2, LFPLUS_REL_CCS = 2 /* the row-wise residual of lfplus_ccs_check: the same bit */, LFPLUS_REL_V = 4, LFPLUS_REL_NORM = 8 };
/* R_ComR1CS (src/r1cs.rs:21-60): cm_f = A f (cm_f NULL: not checked) and (M_A f) o (M_B f) = M_C f row by row in Z_p[X]/(X^16 + 1), for the three n x n
 * matrices that act on f (r1cs_decomposed_square; rowptr NULL: the resident ones, which must number 3).  *first_bad (may be NULL) = the smallest row with a
 * non-zero residual in any of its 16 coefficients, n when every row holds.  The residual is fused: the three product tables are never written. */
int lfplus_r1cs_check(lfplus_ctx *ctx, const uint64_t *cm_f, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val, uint64_t bound,
                      unsigned *failed, uint64_t *first_bad, uint64_t *absmax);
/* R_LinB (src/lin.rs:29-40; built at decomp.rs:76-91, r1cs.rs:119-130): cm_f = A f (kappa*16 words; NULL: not checked) and, for both points pt in {a, b},
 * v[0][pt] = mle(f)(r_pt), v[1 + j][pt] = mle(M_j f)(r_pt).  r_a / r_b: log2(n) ring elements each and v: (1 + nM)*2*16 words, both as lfplus_decompose lays
 * them out (v0); nM matrices (rowptr NULL: the resident ones).  Points whose coordinates are all ring constants (PlusProver's always are) with
 * constant-coefficient matrices take one pass over f; anything else runs through lfplus_decompose's fix_variables tables (correct, not fast). */
int lfplus_linb_check(lfplus_ctx *ctx, const uint64_t *cm_f, const uint64_t *r_a, const uint64_t *r_b, uint32_t nM, const uint32_t *const *rowptr,
                      const uint32_t *const *col, const uint64_t *const *val, const uint64_t *v, uint64_t bound, unsigned *failed, uint64_t *absmax);

/* Matrix::try_mul_vec: out (kappa*16 words) = A * v for a general vector of n ring elements (host pointer) */
int lfplus_commit(lfplus_ctx *ctx, const uint64_t *v, uint64_t n, uint64_t *out);

/* utils::tensor(r) over the base field: out has 2^n words (n <= 28); utils::tensor_product: out has m*n words (or the non-empty side) */
int lfplus_tensor(lfplus_ctx *ctx, const uint64_t *r, uint32_t n, uint64_t *out);
int lfplus_tensor_product(lfplus_ctx *ctx, const uint64_t *a, uint64_t m, const uint64_t *b, uint64_t n, uint64_t *out);

/* ---- the transcript-driven part: PoseidonTranscript<RqPoly>, monomial set check, range check (prover on the GPU, verifier on the host) ----
 * PoseidonTranscript::empty::<FrogPoseidonConfig>() (src/transcript.rs:20-78; table cyclotomic-rings/src/rings/poseidon/frog.rs): a host
 * object.  absorb = Transcript::absorb / absorb_slice (16 words per ring element), challenge = get_challenge (ONE F_p word: RqPoly's base ring
 * has extension degree 1; squeezed and absorbed back), squeeze_bytes as arkworks (7 bytes per element), short_challenge =
 * utils::short_challenge(128, ..) (utils.rs:87-101). */
typedef struct lfplus_transcript lfplus_transcript;
lfplus_transcript *lfplus_transcript_new(void);
lfplus_transcript *lfplus_transcript_clone(const lfplus_transcript *t);
void lfplus_transcript_free(lfplus_transcript *t);
int lfplus_transcript_absorb(lfplus_transcript *t, const uint64_t *ring, size_t count);
int lfplus_transcript_challenge(lfplus_transcript *t, uint64_t *out);
int lfplus_transcript_squeeze_bytes(lfplus_transcript *t, size_t n, uint8_t *out);
int lfplus_short_challenge(lfplus_transcript *t, uint64_t *out16);
int lfplus_poseidon_params(uint64_t *ark720, uint64_t *mds576);   /* the regenerated Frog table (checksummed against the reference's) */
int lfplus_poseidon_permute(uint64_t *state24, int plain);        /* one permutation; plain = 1: the textbook form, 2: the scalar sparse form, 0: what the transcript runs (self-tests) */
int lfplus_poseidon_simd(void);                                   /* 1 when the transcript's permutation runs on the host's AVX-512 IFMA lanes (lfp_poseidon_simd.cc) */

/* In::set_check (src/setchk.rs:65-262): nmat matrix sets of n x ncols unit monomials and nvec vector sets of n, n = 2^nvars, as exponent
 * digits (int8 in (-8, 8); LFPLUS_ABSENT = zero entry); nM matrices (n x n, CSR, ring coefficients) for the M_i f rows of Step 3.
 * Outputs: r (nvars words), msgs (nvars * 4 ring elements: the sumcheck messages, constants), e ((1 + nM) * nmat * ncols ring elements,
 * e[q][set][column]), b (nvec ring elements).  The transcript advances exactly as the reference's. */
int lfplus_set_check(lfplus_ctx *ctx, lfplus_transcript *t, uint32_t nvars, const int8_t *mat_digits, uint32_t nmat, uint32_t ncols, const int8_t *vec_digits,
                     uint32_t nvec, uint32_t nM, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val, uint64_t *r_out,
                     uint64_t *msgs, uint64_t *e_out, uint64_t *b_out);
/* Out::verify (setchk.rs:266-340), host only.  LFPLUS_OK, or LFPLUS_E_REJECT with *stage = 1 / 2 (sumcheck) or 3 (final evaluation). */
int lfplus_set_check_verify(lfplus_transcript *t, uint32_t nvars, uint32_t nmat, uint32_t ncols, uint32_t nvec, uint32_t nM, const uint64_t *msgs, const uint64_t *e,
                            const uint64_t *b, uint64_t *r_out, int *stage);
/* Rg::range_check (src/rgchk.rs:81-186) over L instances: ctxs[l] holds witness f_l and its lfplus_rg_from_f results (same device, n = 2^nvars,
 * k).  Outputs: the set check's r, msgs, e ((1 + nM) * (L k) * 16 ring elements), b (L), and per instance v (16 words), a (1 + nM words),
 * bb (1 + nM ring elements: DcomEvals::b), c (1 + nM ring elements). */
int lfplus_range_check(lfplus_ctx *const *ctxs, uint32_t L, lfplus_transcript *t, uint32_t nM, const uint32_t *const *rowptr, const uint32_t *const *col,
                       const uint64_t *const *val, uint64_t *r_out, uint64_t *msgs, uint64_t *e_out, uint64_t *b_out, uint64_t *v_out, uint64_t *a_out,
                       uint64_t *bb_out, uint64_t *c_out);
/* Dcom::verify (rgchk.rs:193-258), host only: stages 1-3 set check, 4 ct(psi b) != a, 5 ct(psi sum_i (d/2)^i u_i) != v / c */
int lfplus_range_check_verify(lfplus_transcript *t, uint32_t nvars, uint32_t L, uint32_t k, uint32_t nM, const uint64_t *msgs, const uint64_t *e, const uint64_t *b,
                              const uint64_t *v, const uint64_t *a, const uint64_t *bb, const uint64_t *c, uint64_t *r_out, int *stage);
/* Cm::prove (src/cm.rs:56-347) over L resident instances (as lfplus_range_check; ell = DecompParameters::l): the range check, the folding
 * challenges s (3) and s' (k d), h = M_f s' and comh, the two degree-2 ring-valued sumcheckers, the folded witness g = s0 tau + s1 m_tau + s2 f + h
 * and the folded instance ComX (cm.rs:545-580).  Outputs: r .. c_out as lfplus_range_check; comh (L x kappa ring elements); pa / pb (nvars x 3 ring
 * elements: the sumcheck messages); ea / eb (L x (4 + 4 nM) ring elements in the reference's table order: tau, m_tau, f, h, then per matrix M tau,
 * M m_tau, M f, M h); cm_g (L x kappa); ro (ro_a | ro_b, 2 x nvars words); vo (L x (1 + nM) x 2).  g stays on the device in ctxs[l]
 * (lfplus_cm_read_g: n ring elements); g_out may be null or receive L x n ring elements.  LFPLUS_E_ARG when t0 does not fit n (the reference panics). */
int lfplus_cm_prove(lfplus_ctx *const *ctxs, uint32_t L, lfplus_transcript *t, uint32_t ell, uint32_t nM, const uint32_t *const *rowptr, const uint32_t *const *col,
                    const uint64_t *const *val, uint64_t *r_out, uint64_t *msgs, uint64_t *e_out, uint64_t *b_out, uint64_t *v_out, uint64_t *a_out, uint64_t *bb_out,
                    uint64_t *c_out, uint64_t *comh, uint64_t *pa, uint64_t *pb, uint64_t *ea, uint64_t *eb, uint64_t *cm_g, uint64_t *ro, uint64_t *vo,
                    uint64_t *g_out);
int lfplus_cm_read_g(lfplus_ctx *ctx, uint64_t *g_out);
/* CmProof::verify (cm.rs:349-543), host only.  fcoms[l] = cm_f | C_Mf | cm_mtau of instance l (kappa ring elements each).  LFPLUS_OK: accepted, and
 * cm_g / ro / vo are the folded instance recomputed from the proof.  LFPLUS_E_REJECT with *stage = 1-5 (range check), 6 (a sumcheck round),
 * 7 (t0 does not fit n), 8 (final evaluation of a sumchecker) */
int lfplus_cm_verify(lfplus_transcript *t, uint32_t nvars, uint32_t L, uint32_t k, uint32_t ell, uint32_t kappa, uint32_t nM, const uint64_t *const *fcoms,
                     const uint64_t *msgs, const uint64_t *e, const uint64_t *b, const uint64_t *v, const uint64_t *a, const uint64_t *bb, const uint64_t *c,
                     const uint64_t *comh, const uint64_t *pa, const uint64_t *pb, const uint64_t *ea, const uint64_t *eb, uint64_t *cm_g, uint64_t *ro,
                     uint64_t *vo, int *stage);

/* The constraint-system matrices (n x n, CSR, ring coefficients) made resident once: every entry point that takes (nM, rowptr, col, val) uses them when
 * rowptr is NULL (nM must equal their number; for the multi-instance calls they are taken from ctxs[0]).  lfplus_set_matrices(ctx, n, 0, ..) drops them. */
int lfplus_set_matrices(lfplus_ctx *ctx, uint64_t n, uint32_t nM, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val);
int lfplus_share_matrices(lfplus_ctx *ctx, lfplus_ctx *from);   /* use `from`'s resident matrices (same device, no copy; reference-counted) */
/* ComR1CS::linearize (src/r1cs.rs:76-139) on the resident witness f (lfplus_set_witness; n = 2^nvars ring elements) and the R1CS matrices A, B, C
 * (n x n, CSR, ring coefficients): g_q = M_q f, the degree-3 ring-valued sumcheck of eq(r, x) (g_A g_B - g_C)(x), evaluations at ro.
 * Outputs: msgs (nvars x 4 ring elements), ro (nvars words), evals = v | va | vb | vc (4 ring elements). */
int lfplus_r1cs_linearize(lfplus_ctx *ctx, lfplus_transcript *t, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val, uint64_t *msgs,
                          uint64_t *ro, uint64_t *evals);
/* ComR1CSProof::verify (r1cs.rs:141-162), host only: LFPLUS_E_REJECT with *stage = 1 (a sumcheck round) or 2 (e (va vb - vc) != s; the reference asserts) */
int lfplus_r1cs_verify(lfplus_transcript *t, uint32_t nvars, const uint64_t *msgs, const uint64_t *evals, uint64_t *ro, int *stage);
/* DecompProof::verify (src/decomp.rs:101-123), host only: *stage = 1 (C0 + B C1 != cm_f) or 2 (v0 + B v1 != v over `count` pairs of ring elements) */
int lfplus_decomp_verify(const uint64_t *C0, const uint64_t *C1, uint32_t kappa, const uint64_t *v0, const uint64_t *v1, uint32_t count, const uint64_t *cm_f,
                         const uint64_t *v, uint64_t B, int *stage);
/* Mlin::mlin (src/mlin.rs:42-107) over the L resident witnesses of ctxs (same commitment matrix, n, device): RgInstance::from_f(b, k, l) on each, Cm::prove
 * (outputs as lfplus_cm_prove), then the folded LinB2: cm_g_sum (kappa ring elements) and vo_sum ((1 + nM) x 2) on the host, g = sum_l g_l on the device where
 * it REPLACES ctxs[0]'s resident witness (PlusProver::prove hands it to Decomp::decompose: plus.rs:90-95).  fcoms_out (may be null): L x 3 x kappa ring
 * elements, cm_f | C_Mf | cm_mtau per instance (what CmProof::verify needs). */
int lfplus_mlin(lfplus_ctx *const *ctxs, uint32_t L, lfplus_transcript *t, uint64_t b, uint32_t k, uint32_t l, uint32_t nM, const uint32_t *const *rowptr,
                const uint32_t *const *col, const uint64_t *const *val, uint64_t *r_out, uint64_t *msgs, uint64_t *e_out, uint64_t *b_out, uint64_t *v_out,
                uint64_t *a_out, uint64_t *bb_out, uint64_t *c_out, uint64_t *comh, uint64_t *pa, uint64_t *pb, uint64_t *ea, uint64_t *eb, uint64_t *cm_g,
                uint64_t *ro, uint64_t *vo, uint64_t *fcoms_out, uint64_t *cm_g_sum, uint64_t *vo_sum);

/* ---- PlusProver / PlusVerifier as objects (src/plus.rs:15-146) and the flat PlusProof --------------------------------------------------------------
 * PlusParameters (plus.rs:43-47) with LinParameters and DecompParameters flattened: kappa (rows of A), the digit base b, k digits and l gadget digits of the
 * range check, and the decomposition base B of Decomp::decompose (also the base of ComR1CS::new's gadget decomposition of z). */
typedef struct { uint32_t kappa, k, l; uint64_t b, B; } lfplus_params;

/* The flat PlusProof: canonical u64 words, LFPLUS_PROOF_HEADER words of header and then the fields back to back in ONE fixed order
 * (nvars = log2 n, per = 4 + 4 nM, d = 16; sizes in words):
 *   header        LFPLUS_PROOF_MAGIC, L, nfresh, nvars, k, l, kappa, nM
 *   per fresh instance i < nfresh (ComR1CSProof, r1cs.rs:62-74)
 *     msgs        nvars * 4 * d          r        nvars          evals    4 * d
 *   CmProof (cm.rs:24-54), in the order lfplus_mlin takes the pointers
 *     r           nvars                  msgs     nvars * 4 * d  e        (1 + nM) * L * k * d * d
 *     b           L * d                  v        L * d          a        L * (1 + nM)
 *     bb          L * (1 + nM) * d       c        L * (1 + nM) * d
 *     comh        L * kappa * d          pa       nvars * 3 * d  pb       nvars * 3 * d
 *     ea          L * per * d            eb       L * per * d
 *     cm_g        L * kappa * d          ro       2 * nvars      vo       L * (1 + nM) * 2 * d
 *     fcoms       L * 3 * kappa * d      (cm_f | C_Mf | cm_mtau per instance)
 *   LinB2X (mlin.rs:21-40)
 *     cm_g        kappa * d              ro       2 * nvars      vo       (1 + nM) * 2 * d
 *   DecompProof (decomp.rs:24-30)
 *     C0, C1      kappa * d each         v0, v1   (1 + nM) * 2 * d each
 * L = accumulated + fresh instances folded by the prove (2 + nfresh, or nfresh for the first).  lfplus_proof_fields = 3 nfresh + 24 is the number of fields,
 * lfplus_proof_len the total length in words (0: parameters outside the envelope), lfplus_proof_layout writes the offset (in words from the start of the
 * buffer) and the length of every field in the order above (nfields must equal lfplus_proof_fields(nfresh)).  Envelope: n = 2^nvars, 1 <= nvars <= 32,
 * 1 <= L, nfresh <= L <= 4096, 1 <= k <= 16, 1 <= l <= 64, 1 <= kappa <= 64, nM <= 64.  The header is there to be CHECKED: a verifier compares it with its own
 * parameters and never sizes anything from it. */
#define LFPLUS_PROOF_HEADER 8
#define LFPLUS_PROOF_MAGIC 0x4C46504C55533031ULL   /* the bytes "LFPLUS01", most significant first (a canonical word: below p) */
uint32_t lfplus_proof_fields(uint32_t nfresh);
uint64_t lfplus_proof_len(const lfplus_params *params, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh);
int lfplus_proof_layout(const lfplus_params *params, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh, uint64_t *offsets, uint64_t *lengths, uint32_t nfields);

/* PlusProver::init (plus.rs:55-74) on one device: 2 + ncomp contexts, the commitment matrix A (kappa x n x 16 words; NULL: generated on the device from `seed`,
 * lfplus_matrix_generate) and the nM constraint-system matrices (n x n, CSR, as lfplus_set_matrices) installed in the first and shared with the rest.  The
 * instances a prover folds are ComR1CS over these matrices (every reference use has M = cr1cs.x.matrices()), so nM must be 3.  The transcript is BORROWED: the
 * caller keeps ownership, it must outlive the prover and is advanced by lfplus_prover_prove only.  Unsharded only (a column-sharded prover is built from the
 * context-level calls).  The accumulator (F0, F1) of a prove stays on the device, in the first two contexts, as input of the next prove.
 *
 * State machine.  ingest / set_instances name the fresh instances of the NEXT prove (one of the two, once per prove: a second call before the prove is
 * LFPLUS_E_ARG); more instances than free contexts (ncomp after the first prove, 2 + ncomp before it) is LFPLUS_E_ARG and touches nothing.  An error INSIDE
 * ingest, set_instances or prove leaves witnesses half-installed or the Fiat-Shamir transcript half-advanced: the prover is then FAILED and every later call
 * except lfplus_prover_destroy and lfplus_prover_last_error returns LFPLUS_E_ARG with a message.  Shape errors of a call (a NULL pointer, m k != n, a wrong
 * proof_words) are refused before anything is touched and do not fail the prover.  Host memory that cannot be had ends a call with LFPLUS_E_HIP (no C++ exception
 * leaves the library).  One thread per prover at a time. */
typedef struct lfplus_prover lfplus_prover;
int lfplus_prover_create(int device, const lfplus_params *params, const uint64_t *A, uint64_t seed, uint64_t n, uint32_t nM, const uint32_t *const *rowptr,
                         const uint32_t *const *col, const uint64_t *const *val, uint32_t ncomp, lfplus_transcript *transcript, lfplus_prover **out);
/* releases the contexts (their scratch goes to the process-wide cache: lfplus_scratch_trim) and joins the upload thread; the transcript is not freed */
void lfplus_prover_destroy(lfplus_prover *prover);
const char *lfplus_prover_last_error(const lfplus_prover *prover);
/* ComR1CS::new for `count` fresh instances from their short witnesses z[i] (m ring elements each, n = m k; l_in is the instance's public-input length, kept for
 * the reference's signature and not used by the fold): lfplus_witness_from_z(B, k) in the contexts the next prove folds from; cm_f_out (may be NULL) receives
 * count x kappa x 16 words. */
int lfplus_prover_ingest(lfplus_prover *prover, const uint64_t *const *z, uint32_t count, uint64_t m, uint32_t l_in, uint64_t *cm_f_out);
/* The same from host witnesses f[i] (n ring elements each).  Returns at once: a worker thread uploads them one after the other, and the next prove linearizes
 * the instances as they arrive (only the first upload is exposed).  f[i] is BORROWED until that prove -- or lfplus_prover_destroy -- returns; an upload that
 * fails (a non-canonical word) is reported by the prove.  cm_f (may be NULL, as may any cm_f[i]): the instances' commitments, kappa x 16 words each, copied;
 * the prove compares them with the commitments it computes (fcoms) and fails on a difference. */
int lfplus_prover_set_instances(lfplus_prover *prover, const uint64_t *const *f, const uint64_t *const *cm_f, uint32_t count);
/* PlusProver::prove (plus.rs:77-108): RgInstance::from_f of the accumulator halves and of every fresh instance on the contexts' second streams, the
 * linearization of each fresh instance as it arrives, Mlin::mlin, Decomp::decompose with the parts left in the first two contexts.  Writes one flat proof:
 * proof_words must equal lfplus_proof_len(params, n, nM, L, nfresh) for this prove's L and nfresh (otherwise LFPLUS_E_ARG, nothing touched). */
int lfplus_prover_prove(lfplus_prover *prover, uint64_t *proof, uint64_t proof_words);
/* the accumulator of the last prove read back: n x 16 words each (either may be NULL) */
int lfplus_prover_accumulator(lfplus_prover *prover, uint64_t *F0, uint64_t *F1);
/* Are the two halves of the accumulator valid LinB instances (lfplus_linb_check where they live) for `proof`, the flat proof of the LAST prove?  Half i = (F_i,
 * C_i, v_i) at the points linb2x.ro, ||F_i||_inf < bound (0: not checked).  ok[i] = 1 / 0, failed[i] = the LFPLUS_REL_* bits, absmax[i] as lfplus_linb_check.
 * LFPLUS_OK when both hold, LFPLUS_E_REJECT when one does not (all six outputs are written in both cases).  Read-only. */
int lfplus_prover_decide(lfplus_prover *prover, const uint64_t *proof, uint64_t proof_words, uint64_t bound, int *ok, unsigned *failed, uint64_t *absmax);
/* PlusVerifier::verify (plus.rs:132-143), host only: no GPU, no context.  The verifier's OWN statement is (params, n, nM, L, nfresh); a buffer whose length or
 * header disagrees with it, or a NULL proof, is LFPLUS_E_ARG before any word of a field is read.  Then lfplus_r1cs_verify per fresh instance, lfplus_cm_verify,
 * lfplus_decomp_verify on the borrowed transcript.  LFPLUS_E_REJECT: *which = i < nfresh for the i-th ComR1CSProof, nfresh for the CmProof, nfresh + 1 for the
 * DecompProof, and *stage = that verifier's stage (either may be NULL). */
int lfplus_verify(const lfplus_params *params, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh, lfplus_transcript *transcript, const uint64_t *proof,
                  uint64_t proof_words, int *which, int *stage);

/* ---- device-resident callers: the O(n) arrays as DEVICE memory ------------------------------------------------------------------------------------------
 * Every entry point above takes host pointers.  A `_dev` twin has the parameter list of its call and its results, word for word, but the O(n) arrays -- the
 * witness f, the short witness z, the vector v of lfplus_commit, f_out, the halves F0 / F1 -- are memory of the CONTEXT'S DEVICE (hipMalloc, a torch tensor,
 * ...).  Everything small stays a host pointer: cm_f, out, C0 / C1, v0 / v1, r_a / r_b, the CSR arrays, the arrays OF pointers (z, f of the prover calls: host
 * arrays of device pointers; cm_f of lfplus_prover_set_instances_dev: host arrays throughout).  No twin exists for the commitment matrix (set once;
 * lfplus_matrix_generate avoids the upload), for lfplus_rg_read, the digit arrays of the set check / range check or the relation checks.
 *   Layout: that of the host ABI -- coefficient form, 16 canonical little-endian u64 words per ring element, AoS.  It is also the library's resident layout:
 * lfplus_witness_from_z_dev, lfplus_commit_dev and lfplus_decompose_dev read and write the caller's array in place (no staging copy; lfplus_decompose_dev
 * allocates no scratch for a half the caller receives), lfplus_set_witness_dev and lfplus_prover_set_instances_dev copy it once with the kernel that tests its
 * words, lfplus_get_witness_dev and lfplus_prover_accumulator_dev are one device-to-device copy.
 *   Pointer checks, after the twin's own argument and state checks and before anything is touched or enqueued: the array is not NULL (F0 / F1 may be, as in the
 * host calls), hipPointerGetAttributes reports unmanaged device memory of the context's device, hipMemGetAddressRange shows ONE allocation covering every byte
 * the call touches, and the pointer is 16-BYTE aligned (lfhip.h asks for 8: the kernels of this slice use 16-byte vector accesses; a view of whole ring elements
 * into any allocation satisfies it).  Anything else -- a host or pinned pointer, another device, a misaligned pointer, a range that runs off its allocation -- is
 * LFPLUS_E_ARG with a message in lfplus_last_error / lfplus_prover_last_error: no kernel is launched on such a pointer, no output is written, the context keeps
 * the resident witness and the lfplus_rg_from_f results it had, the prover is not FAILED and stays usable.  (lfplus_witness_from_z_dev keeps the witness on
 * EVERY refusal of its checks; its host twin drops it.)  A sharded context (a transport or lfplus_set_sharding_model) refuses every _dev call the same way.
 *   Canonical words: the host cannot inspect device data, so the device does.  lfplus_set_witness_dev and lfplus_witness_from_z_dev behave as their twins: a
 * word >= p is LFPLUS_E_ARG and the context is left WITHOUT a resident witness.  lfplus_commit_dev: LFPLUS_E_ARG, `out` is not written, the resident witness is
 * untouched.
 *   Overlap: F0 and F1 of lfplus_decompose_dev / lfplus_prover_accumulator_dev must not overlap each other (LFPLUS_E_ARG); read-only inputs may alias each other.
 *   Ordering: a _dev call reads its inputs on the context's stream.  The caller guarantees that they are complete -- by synchronising its own stream, or by
 * lfplus_ctx_wait_stream(ctx, stream) first: it records an event on `stream` (a hipStream_t; NULL = the default stream) and makes both streams of the context
 * wait for it, without blocking the host and without touching `stream` otherwise; lfplus_prover_wait_stream does so for every context of the prover (and joins
 * an upload thread that still writes into them).  A _dev call returns after the context's stream is synchronised: device outputs are complete and the inputs
 * are free for reuse on return.
 *   After a failure other than the refusals above (LFPLUS_E_HIP, a non-canonical word) the device outputs of the call are undefined; the context or prover is
 * in the state its host twin leaves (no resident witness; an error INSIDE lfplus_prover_ingest_dev / lfplus_prover_set_instances_dev makes the prover FAILED).
 *   No upload thread: lfplus_prover_set_instances_dev copies and checks on the calling thread and returns when the instances are resident -- f[i] is NOT
 * borrowed after it returns, a non-canonical word is reported by THIS call (LFPLUS_E_ARG, prover FAILED), and the following prove finds every instance arrived.
 *   Pending work: a pending lfplus_rg_from_f_async pass is joined before the witness it reads is overwritten, exactly as in the twins. */
int lfplus_ctx_wait_stream(lfplus_ctx *ctx, void *hip_stream);
int lfplus_set_witness_dev(lfplus_ctx *ctx, const uint64_t *f, uint64_t n);
int lfplus_witness_from_z_dev(lfplus_ctx *ctx, const uint64_t *z, uint64_t m, uint64_t b, uint32_t k, uint64_t *cm_f);
int lfplus_commit_dev(lfplus_ctx *ctx, const uint64_t *v, uint64_t n, uint64_t *out);
int lfplus_get_witness_dev(lfplus_ctx *ctx, uint64_t *f_out /* n * 16 words */, uint64_t n);
int lfplus_decompose_dev(lfplus_ctx *ctx, uint64_t B, const uint64_t *r_a, const uint64_t *r_b, uint32_t nm, const uint32_t *const *rowptr,
                         const uint32_t *const *col, const uint64_t *const *val, uint64_t *F0, uint64_t *F1, uint64_t *C0, uint64_t *C1, uint64_t *v0,
                         uint64_t *v1);
int lfplus_prover_wait_stream(lfplus_prover *prover, void *hip_stream);
int lfplus_prover_ingest_dev(lfplus_prover *prover, const uint64_t *const *z, uint32_t count, uint64_t m, uint32_t l_in, uint64_t *cm_f_out);
int lfplus_prover_set_instances_dev(lfplus_prover *prover, const uint64_t *const *f, const uint64_t *const *cm_f, uint32_t count);
int lfplus_prover_accumulator_dev(lfplus_prover *prover, uint64_t *F0, uint64_t *F1);

/* ---- MLSumcheck::prove_as_subprotocol / verify_as_subprotocol over ANY sum of products of MLE tables (latticefold utils/sumcheck.rs:53-104,
 * sumcheck/prover.rs:56-162, sumcheck/verifier.rs:92-257; the VirtualPolynomial of sumcheck/utils.rs:24-75) on the Frog ring: the counterpart of
 * lf_mlsumcheck_* (lfhip_sumcheck.h), field for field.  Every sumcheck of latticefold-plus is this one MLSumcheck with another comb function (r1cs.rs:90-95,
 * cm.rs, setchk.rs); the three the slice runs keep their specialised kernels and digests, this is the call for every OTHER constraint shape over RqPoly.
 *      g(x) = sum_{i < nterms} coef_i * prod_{k in [term_off[i], term_off[i+1])} T_{term_idx[k]}(x),      x in {0,1}^nvars,
 * with negacyclic products in Z_p[X]/(X^16 + 1).  Tables are ntables x 2^nvars GENERAL ring elements in the layout of this header (coefficient form, 16 canonical
 * words per element, AoS; table j at tables + j * 2^nvars * 16); entry x of a table has variable 1 in bit 0 of x (DenseMultilinearExtension: the first round
 * fixes the lowest bit).  A constant-polynomial table (eq(r, .); lfplus_build_eq_device makes it) costs a full ring table and full products.  A challenge is ONE F_p word (RqPoly's base ring has
 * extension degree 1): fix_variables is lo + r (hi - lo), coefficient by coefficient.
 *   Independence.  The state and the buffers of this sumcheck are the context's own and nothing else's: it runs on a BARE context (no matrix, no witness), and on
 * a loaded one it neither reads nor writes the resident witness, the lfplus_rg_from_f results, a pending lfplus_rg_from_f_async pass or the resident matrices.
 * The caller's tables are never written, in either memory space.  lfplus_mlsumcheck_begin while a generic sumcheck is active replaces it; so does
 * lfplus_mlsumcheck_prove, which leaves none behind.
 *   Refusals of begin / prove, every one LFPLUS_E_ARG with a message in lfplus_last_error, in this order: a NULL argument; a table index >= ntables; term_off that
 * does not start at 0 or is not strictly increasing (every term has at least one factor); a coefficient word >= p; anything outside the envelope stated on the
 * fields below; a sharded context (a transport or lfplus_set_sharding_model); [_device: the pointer checks of the _dev section above;] a table word >= p (host tables
 * are tested on the host before anything is enqueued, device tables by the first kernel that reads them: the flag it raises comes home before begin returns).
 * Without a device: LFPLUS_E_NO_DEVICE (also for the NULL context such a caller holds).  Of the split form, LFPLUS_E_ARG as well: lfplus_mlsumcheck_round before
 * a begin, with r_prev NULL in a later round or non-NULL in round 1, or after nvars rounds; lfplus_mlsumcheck_final before the last round; a challenge >= p.
 *   After any refusal the context is usable.  A begin refused by the checks above leaves a sumcheck in progress as it was -- except one refused after the tables
 * were touched (a device word >= p, an allocation failure: LFPLUS_E_HIP): that leaves none, and the next round is refused.  lfplus_mlsumcheck_prove refuses
 * everything above before its first absorb: the transcript is untouched then. */
typedef struct {
    uint32_t nvars;            /* m = 2^nvars entries per table, 1 <= nvars <= 28 (the slice's n limit) */
    uint32_t ntables;          /* T, 1..16 */
    uint32_t nterms;           /* q, 1..16 */
    uint32_t degree;           /* the degree the prover absorbs and sends degree+1 evaluations for; max_i |S_i| <= degree <= 8 */
    const uint32_t *term_off;  /* q+1 offsets into term_idx; every term has 1..8 factors; term_off[q] <= 64 */
    const uint32_t *term_idx;  /* table indices < T; an index may repeat inside a term (a square) and across terms */
    const uint64_t *coef;      /* q ring elements, 16 canonical words each, any value including 0 */
} lfplus_vpoly;
/* The split form (the caller's transcript stays in charge between the rounds).  begin copies the descriptor, the coefficients and the tables into buffers of
 * the context: the caller's arrays are free again when the call returns. */
int lfplus_mlsumcheck_begin(lfplus_ctx *ctx, const lfplus_vpoly *poly, const uint64_t *tables /* T x m x 16 words */);
/* the same with `tables` in memory of the context's device (spelled _device, as lf_mlsumcheck_begin_device is), under every rule of the _dev section above (unmanaged memory of the context's device, ONE allocation
 * covering T * m * 128 bytes, 16-byte alignment, ordering by lfplus_ctx_wait_stream, return after the context's stream is synchronised).  The device layout is
 * the resident layout: the array is copied once, by the kernel that tests its words, and is free again on return */
int lfplus_mlsumcheck_begin_device(lfplus_ctx *ctx, const lfplus_vpoly *poly, const uint64_t *tables /* device */);
/* round i = 1 .. nvars: fixes the previous variable at r_prev, then evaluates the round polynomial at 0 .. degree */
int lfplus_mlsumcheck_round(lfplus_ctx *ctx, const uint64_t *r_prev /* ONE word; NULL in round 1 */, uint64_t *evals_out /* (degree+1) x 16 words */);
/* valid after nvars rounds: fixes the last variable at r_last and returns every table's value at the whole point.  DEVIATION from ProverState
 * (sumcheck/prover.rs), as lf_mlsumcheck_final: the reference leaves the MLEs fixed nvars - 1 times and each caller evaluates them next */
int lfplus_mlsumcheck_final(lfplus_ctx *ctx, const uint64_t *r_last /* one word */, uint64_t *evals_out /* T x 16 words */);
/* drops the state; always LFPLUS_OK (LFPLUS_E_ARG for a NULL context) */
int lfplus_mlsumcheck_end(lfplus_ctx *ctx);
/* prove_as_subprotocol in one call: absorb(nvars), absorb(degree) as constant polynomials, then per round absorb_slice(the degree+1 evaluations), get_challenge,
 * absorb(the challenge as a constant polynomial) -- the schedule of every sumcheck of the slice.  msgs_out: nvars x (degree+1) x 16 words (the Proof);
 * point_out: the nvars challenges; final_out (may be NULL): the T table values at the point, as lfplus_mlsumcheck_final.  The _device form reads the caller's
 * device array IN PLACE (rounds 1 and 2; the fixed tables of round 2 onwards go to scratch of the context): no staging copy */
int lfplus_mlsumcheck_prove(lfplus_ctx *ctx, lfplus_transcript *t, const lfplus_vpoly *poly, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out,
                            uint64_t *final_out);
int lfplus_mlsumcheck_prove_device(lfplus_ctx *ctx, lfplus_transcript *t, const lfplus_vpoly *poly, const uint64_t *tables /* device */, uint64_t *msgs_out,
                                uint64_t *point_out, uint64_t *final_out);
/* verify_as_subprotocol on the host: no context, no GPU.  claimed_sum: one ring element; msgs: nvars x (degree+1) ring elements; point_out: nvars words;
 * expected_out: one ring element, the subclaim's expected evaluation g(point) (written on LFPLUS_OK only).  The transcript runs over ALL rounds first, the checks
 * follow (verifier.rs:92-139); interpolation is the coefficient-wise Lagrange form on the nodes 0 .. degree -- the one host body lfplus_r1cs_verify and
 * lfplus_cm_verify run their sumcheck rounds through.  LFPLUS_OK with *round = -1, or LFPLUS_E_REJECT with *round = the index (from 0) of the first round whose
 * p(0) + p(1) is not the running claim (round may be NULL).  A NULL argument, nvars == 0 or > 28, degree == 0 or > 8, a word >= p in claimed_sum or msgs ->
 * LFPLUS_E_ARG, the transcript untouched */
int lfplus_mlsumcheck_verify(lfplus_transcript *t, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum, const uint64_t *msgs, uint64_t *point_out,
                             uint64_t *expected_out, int *round);

/* ---- ring arithmetic on arrays: the negacyclic product and the resident matrices as calls of their own (the counterparts of lf_ring_mul / lf_spmv on the Frog
 * ring; the oracle's lfp_ring_mul).  With lfplus_tensor and lfplus_mlsumcheck_prove_device they take a constraint shape the slice does not hard-wire from the
 * witness to the proof on the device: g_q = lfplus_spmv_device(q, f), products and residuals of those tables with lfplus_ring_mul_device, linear combinations
 * sum_l s_l f_l with ring (short-challenge) coefficients in the broadcast mode.
 *   Layout as everywhere in this header: coefficient form, 16 canonical little-endian words per element, AoS.  Envelope: 1 <= n_terms <= 64, 1 <= count <= 2^28,
 * mode 0 or 1.  The device forms (spelled _device, as lfplus_mlsumcheck_begin_device is) take a, out, x, y -- and b in mode 0 -- as memory of the context's device
 * under every rule of the "device-resident callers" section above (unmanaged memory of the context's device, ONE allocation covering every byte, 16-byte
 * alignment, ordering by lfplus_ctx_wait_stream, return after the context's stream is synchronised); b of mode 1 is small and stays a HOST pointer.
 *   Independence, as lfplus_mlsumcheck_*: the calls run on a bare context (lfplus_ring_mul needs no matrix and no witness) and on a loaded one neither read nor
 * write the resident witness, the lfplus_rg_from_f results, a pending lfplus_rg_from_f_async pass or an active generic sumcheck.  Inputs are never written.
 *   Aliasing: a and b may alias each other (a square).  out may be EXACTLY a (or exactly b in mode 0) when n_terms == 1; any other overlap of out with an input
 * range is refused with nothing launched, in both memory spaces.  y overlapping x in any way is refused: the product gathers.
 *   Refusals, every one LFPLUS_E_ARG with a message in lfplus_last_error, in this order: a NULL context (tested before any device is touched: the answer on a
 * machine without a GPU as well); a NULL array; n_terms, count or mode outside the envelope; [lfplus_spmv: no resident matrices, j >= their number, n != the
 * resident n;] a sharded context (a transport or lfplus_set_sharding_model); the overlap rules; [_device: the pointer checks;] in mode 1 a word >= p in b (tested
 * on the host); a word >= p in an O(n) input.  The O(n) words are tested on the device by the kernel that reads them and the flag comes home before the call
 * returns: a host out / y is downloaded only when it is down and stays untouched otherwise, a device out / y is undefined then (as that section says for a
 * non-canonical word).  After any refusal the context is usable and nothing resident has changed.
 *   Not built: sharded contexts; an NTT form of the Frog ring (its slot conventions are unpinned and it has no oracle); an int8 matrix-core form of the product. */
#define LFPLUS_MUL_ELEMENTWISE 0   /* b: n_terms x count ring elements */
#define LFPLUS_MUL_BROADCAST   1   /* b: n_terms ring elements, one per term */
/* mode 0: out[x] = sum_{i<n_terms} a_i[x] * b_i[x]; mode 1: out[x] = sum_i a_i[x] * b_i; x < count,
 * negacyclic products in Z_p[X]/(X^16+1); table i of a at a + i*count*16 words */
int lfplus_ring_mul(lfplus_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t n_terms, uint64_t count, int mode, uint64_t *out);
int lfplus_ring_mul_device(lfplus_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t n_terms, uint64_t count, int mode, uint64_t *out);
/* y = M_j x, M_j the j-th matrix of lfplus_set_matrices / lfplus_share_matrices (n x n), x and y n ring elements */
int lfplus_spmv(lfplus_ctx *ctx, uint32_t j, const uint64_t *x, uint64_t n, uint64_t *y);
int lfplus_spmv_device(lfplus_ctx *ctx, uint32_t j, const uint64_t *x, uint64_t n, uint64_t *y);

/* ---- MLE tables on arrays: the eq(r, .) table, evaluations and partial evaluations of tables at a point, and M_j^T v (the counterparts of lf_build_eq,
 * lf_mle_eval_batch, lf_mle_fix_variables and lf_spmv_t on the Frog ring; DenseMultilinearExtension::{evaluate, fix_variables}, utils::mle_helpers build_eq_x_r).
 * With the section above they close the loop of a generic sumcheck on the device: lfplus_build_eq_device makes the eq factor lfplus_mlsumcheck_begin(_device)
 * takes, lfplus_mle_eval_batch_device evaluates tables outside a sumcheck, and w = lfplus_spmv_t_device(j, eq(r, .)) turns u_j = MLE(M_j f)(r) into the one inner
 * product sum_c f[c] * w[c].
 *   Layout as everywhere in this header: coefficient form, 16 canonical little-endian words per element, AoS; table j of `tables` at tables + j * len * 16.  A
 * challenge is ONE F_p word, so a point is nv (nfix) words; entry x of a table has variable 1 in bit 0 of x.  Points are small and stay HOST pointers in both
 * spellings, as does `out` of lfplus_mle_eval_batch.  The device forms (spelled _device, as lfplus_mlsumcheck_begin_device is) take every other array as memory of
 * the context's device under every rule of the "device-resident callers" section above (unmanaged memory of the context's device, ONE allocation covering every
 * byte, 16-byte alignment, ordering by lfplus_ctx_wait_stream, return after the context's stream is synchronised).
 *   Envelope: 1 <= nv <= 28; 1 <= ntables <= 64; lfplus_mle_eval_batch: 1 <= len <= 2^nv, entries from len on count as zero (the ragged form lf_mle_eval_batch
 * has); lfplus_mle_fix_variables: len = 2^nv, 1 <= nfix <= nv.
 *   Exactness: every output word is the canonical value of an exact sum mod p.  Fixing nfix variables in one call gives the words of nfix calls that fix one
 * each (lo + r (hi - lo), coefficient by coefficient); nfix == nv leaves what lfplus_mle_eval_batch returns; a column of lfplus_spmv_t does not depend on the
 * order or the number of its entries.  The eq weights of an evaluation are never materialised as a ring table.
 *   Independence, as lfplus_mlsumcheck_*: lfplus_build_eq, lfplus_mle_eval_batch and lfplus_mle_fix_variables run on a bare context (no matrix and no witness),
 * and on a loaded one none of the eight reads or writes the resident witness, the lfplus_rg_from_f results, a pending lfplus_rg_from_f_async pass or an active
 * generic sumcheck.  Inputs are never written.  lfplus_spmv_t reads the transposed structure the resident matrices carry: it is owned and reference-counted
 * with them (a context that got them through lfplus_share_matrices shares it) and goes when they are replaced.
 *   Refusals, every one LFPLUS_E_ARG with a message in lfplus_last_error, in this order: a NULL context (tested before any device is touched: the answer on a
 * machine without a GPU as well); a NULL array; ntables, len, nv or nfix outside the envelope; [lfplus_spmv_t: no resident matrices, j >= their number, n != the
 * resident n;] a sharded context (a transport or lfplus_set_sharding_model); out overlapping an input range (arrays of one memory space; out of lfplus_spmv_t
 * overlapping v in any way: the product gathers); [_device: the pointer checks;] a word >= p in the point (tested on the host); a word >= p in an O(n) input.
 * The O(n) words are tested on the device by the kernel that reads them and the flag comes home before the call returns: a host out is written only when it is
 * down and stays untouched otherwise, a device out is undefined then (as that section says for a non-canonical word).  After any refusal the context is usable
 * and nothing resident has changed.
 *   Not built: sharded contexts; an NTT form of the Frog ring; a compact (one word per entry) eq output. */
/* out[x] = the constant polynomial eq(point, x) = prod_i (r_i x_i + (1 - r_i)(1 - x_i)) for x < 2^nv: word 0 holds the value, words 1..15 are 0 -- the table
 * lfplus_mlsumcheck_begin(_device) takes as the eq factor */
int lfplus_build_eq(lfplus_ctx *ctx, const uint64_t *point /* nv words */, uint32_t nv, uint64_t *out /* 2^nv x 16 words */);
int lfplus_build_eq_device(lfplus_ctx *ctx, const uint64_t *point /* nv words */, uint32_t nv, uint64_t *out /* 2^nv x 16 words */);
/* out[j] = sum_{x < len} eq(point, x) * T_j[x], coefficient by coefficient: DenseMultilinearExtension::evaluate of ntables tables of GENERAL ring elements */
int lfplus_mle_eval_batch(lfplus_ctx *ctx, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point /* nv words */, uint32_t nv,
                          uint64_t *out /* ntables x 16 words, host */);
int lfplus_mle_eval_batch_device(lfplus_ctx *ctx, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point /* nv words */, uint32_t nv,
                          uint64_t *out /* ntables x 16 words, host */);
/* DenseMultilinearExtension::fix_variables on whole tables: the LOWEST nfix variables at point[0 .. nfix); table j of out at out + j * (len >> nfix) * 16 */
int lfplus_mle_fix_variables(lfplus_ctx *ctx, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point /* nfix words */, uint32_t nfix,
                             uint64_t *out /* ntables x (len >> nfix) x 16 words */);
int lfplus_mle_fix_variables_device(lfplus_ctx *ctx, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point /* nfix words */, uint32_t nfix,
                             uint64_t *out /* ntables x (len >> nfix) x 16 words */);
/* out[c] = sum over the entries (r, c) of M_j of M_j[r][c] * v[r] (negacyclic products), M_j the j-th matrix of lfplus_set_matrices / lfplus_share_matrices
 * (n x n); v and out n GENERAL ring elements */
int lfplus_spmv_t(lfplus_ctx *ctx, uint32_t j, const uint64_t *v, uint64_t n, uint64_t *out);
int lfplus_spmv_t_device(lfplus_ctx *ctx, uint32_t j, const uint64_t *v, uint64_t n, uint64_t *out);

/* ---- gadget maps on arrays: the digit and gadget maps every LatticeFold+ object is built with, as calls of their own (the counterparts of lf_decompose,
 * lf_recompose and lf_linf_check on the Frog ring): Vec<R>::gadget_decompose(b, k) (r1cs.rs:50), decompose_to_vec(b, k) with or without .transpose()
 * (decomp.rs:34, rgchk.rs:271), gadget_recompose / recompose (z = G f: the check DecompProof::verify performs, on arrays), the infinity norm of an array, and
 * SparseMatrix::gadget_decompose(b, k) + pad_rows(n) = r1cs_decomposed_square (r1cs.rs:172-185) from the system as stated over z.  With the three sections above a
 * caller that builds its own relation cuts a table into digits, puts digits back together, bounds a norm and loads a system stated over z without the host.
 *   Layout as everywhere in this header: coefficient form, 16 canonical little-endian words per element, AoS.  The device forms (spelled _device, as
 * lfplus_mlsumcheck_begin_device is) take in / out / v as memory of the context's device under every rule of the "device-resident callers" section above (unmanaged
 * memory of the context's device, ONE allocation covering every byte, 16-byte alignment, ordering by lfplus_ctx_wait_stream, return after the context's stream is
 * synchronised); absmax stays a HOST pointer, as do the CSR arrays of lfplus_set_matrices_gadget.
 *   Envelope: 1 <= count and count * k <= 2^28; 1 <= k <= 64; 2 <= b <= 2^62 (every intermediate of the digit rule then fits an int64; the centred value is below
 * 2^63); layout 0 or 1; lfplus_linf_norm: 1 <= count <= 2^28; lfplus_set_matrices_gadget: n <= 2^32, nnz * k < 2^32 per matrix, nM <= 64, rows <= n, m * k == n.
 *   Decompose: each of the 16 coefficients is centred to (-p/2, p/2), then k steps of the ONE digit rule of this slice are taken (lfp::digit_step on the device,
 * lfp_balanced_digits in the oracle: the division truncates, a remainder with |rem| <= b/2 is kept, a tie keeps the sign of the value; powers of two take the shift
 * path, every other b the division path) and each digit is written as its canonical residue.  A value that does not fit k digits loses what is left, as in the
 * reference and in lfplus_witness_from_z: not an error.  Recompose: out[j] = sum_{i<k} b^i in[digit i of j], coefficient by coefficient mod p, for GENERAL ring
 * elements in every slot (the k powers are computed once on the host); every output word is the canonical value of the exact sum.  It inverts decompose exactly
 * when the value fitted.  lfplus_linf_norm: *absmax = the largest |centred coefficient| over count * 16 words (centred as for the relation checks, which run the
 * same kernel).
 *   lfplus_set_matrices_gadget: nM matrices of rows x m (CSR, ring coefficients, 16 words per non-zero: the system as stated over z) become the context's resident
 * matrices exactly as after lfplus_set_matrices(ctx, n, nM, pad_rows(gadget_decompose(M_q, b, k), n)): the coefficient c at (r, j) becomes c b^i mod p at
 * (r, j k + i), rows from `rows` on are empty.  Only the short CSR arrays and the short column counts cross PCIe (a k-th of the data; no host product); the device
 * expands them into the complete resident matrix, the transposed structure lfplus_spmv_t reads and the constant-coefficient copies included, and every later call
 * takes the result unchanged: lfplus_spmv, lfplus_spmv_t, lfplus_r1cs_linearize, lfplus_ccs_*, the checks, and the provers through lfplus_share_matrices (the
 * set is reference-counted like any other).  nM == 0 drops the matrices, as lfplus_set_matrices does.  The CSR arrays are validated as lfplus_set_matrices
 * validates them; on ANY failure the matrices that were resident before stay resident.
 *   Independence, as lfplus_mlsumcheck_*: the six array calls run on a bare context (no matrix and no witness), and on a loaded one they neither read nor write the
 * resident witness, the lfplus_rg_from_f results, a pending lfplus_rg_from_f_async pass, the resident matrices or an active generic sumcheck.  Inputs are never written.
 *   Refusals, every one LFPLUS_E_ARG with a message in lfplus_last_error, in this order: a NULL context (tested before any device is touched: the answer on a
 * machine without a GPU as well); a NULL array; anything outside the envelope; a sharded context (a transport or lfplus_set_sharding_model); out overlapping in in
 * any way, with nothing launched (both maps permute); [_device: the pointer checks;] a word >= p in an O(n) input.  The O(n) words are tested on the device by the
 * kernel that reads them and the flag comes home before the call returns: a host out (or *absmax) is written only when it is down and stays untouched otherwise,
 * a device out is undefined then.  After any refusal the context is usable and nothing resident has changed.
 *   Not built: sharded contexts; an int8 output form of the digits (lfplus_rg_read returns the exponent digits of the range check); exp() of digits to dense
 * monomials; a prover constructor that takes the short system (lfplus_prover_create after lfplus_set_matrices_gadget and lfplus_share_matrices already serves it:
 * the prover's contexts share what the first one holds). */
#define LFPLUS_DIGITS_GADGET 0  /* digit i of element j at out[j k + i]: Vec<R>::gadget_decompose(b, k) = what lfplus_witness_from_z makes resident */
#define LFPLUS_DIGITS_PLANES 1  /* digit i of element j at out[i count + j]: decompose_to_vec(b, k).transpose() = F_0, F_1 of lfplus_decompose; D_f order of lfplus_rg_read */
int lfplus_balanced_decompose(lfplus_ctx *ctx, const uint64_t *in /* count */, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out /* count k */);
int lfplus_balanced_decompose_device(lfplus_ctx *ctx, const uint64_t *in /* count */, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out /* count k */);
int lfplus_balanced_recompose(lfplus_ctx *ctx, const uint64_t *in /* count k GENERAL ring elements */, uint64_t count, uint64_t b, uint32_t k, int layout,
                              uint64_t *out /* count */);
int lfplus_balanced_recompose_device(lfplus_ctx *ctx, const uint64_t *in /* count k GENERAL ring elements */, uint64_t count, uint64_t b, uint32_t k, int layout,
                                     uint64_t *out /* count */);
int lfplus_linf_norm(lfplus_ctx *ctx, const uint64_t *v, uint64_t count, uint64_t *absmax /* host */);
int lfplus_linf_norm_device(lfplus_ctx *ctx, const uint64_t *v /* device */, uint64_t count, uint64_t *absmax /* host */);
int lfplus_set_matrices_gadget(lfplus_ctx *ctx, uint64_t rows, uint64_t m, uint64_t b, uint32_t k, uint64_t n, uint32_t nM, const uint32_t *const *rowptr,
                               const uint32_t *const *col, const uint64_t *const *val);

/* ---- committed CCS instances: the linearization of ANY constraint shape sum_i c_i prod_{j in S_i} (M_j f) = 0 as a protocol step of its own, with its own round
 * kernel (lfp_ccs.hip).  The reference has none (its README lists "Support CCS" as the next step of latticefold-plus): this is ComR1CS::linearize /
 * ComR1CSProof::verify (src/r1cs.rs:72-163) generalised in the only way that leaves the R1CS case untouched -- SELF-CONSISTENT, PINNED TO THE REFERENCE AT THE
 * R1CS SHAPE: with t = 3, S = ({0,1},{2}), c = (1, -1) every word of msgs, ro, evals and the transcript state afterwards is that of lfplus_r1cs_linearize.
 *   Shape: t matrices M_0 .. M_{t-1} (n x n, CSR, ring coefficients, as lfplus_set_matrices), q multisets S_i of matrix indices (S_idx[S_off[i] .. S_off[i+1])) and
 * q ring coefficients c_i (16 canonical words each); d = max |S_i|.  An index may repeat inside a multiset (a power) and across multisets (a Plonk-style gate).
 *   Prover, on the resident witness f (n = 2^nvars ring elements): g_j = M_j f; nvars challenges r from the transcript; MLSumcheck::prove_as_subprotocol of
 * eq(r, .) * sum_i c_i prod_{j in S_i} g_j at degree d + 1 (absorbs nvars, d + 1, each round's d + 2 evaluations; draws and re-absorbs the challenge);
 * v = mle(f)(ro), v_j = mle(g_j)(ro); absorbs [v, v_0 .. v_{t-1}] as one slice.  Outputs: msgs (nvars x (d + 2) ring elements), ro (nvars words), evals
 * ((1 + t) ring elements).  The LinB of the instance is (f, cm_f, r = ro at both points, v = evals at both points): what lfplus_mlin -> lfplus_decompose take with nM = t.
 *   Verifier, host only (no context): draws r, verify_as_subprotocol(nvars, d + 1, claimed sum 0), absorbs the evals, accepts iff
 * eq(r, ro) * sum_i c_i prod_{j in S_i} v_j is the expected evaluation.  LFPLUS_E_REJECT with *stage = 1 (a sumcheck round) or 2 (the final identity).
 *   Neither side checks that the instance is satisfied (the reference's prover does not either): the verifier's round 0 and lfplus_ccs_check do.
 *   Refusals, every one LFPLUS_E_ARG (with a message in lfplus_last_error where there is a context) before the transcript or the context is touched, in this
 * order: a NULL argument; t or q outside 1 .. 8; S_off that does not start at 0 or is not strictly increasing (every |S_i| >= 1); a multiset of more than 7
 * indices (d <= 7); S_off[q] > 16; an index >= t; a word of c >= p; [lfplus_ccs_verify: nvars outside 1 .. 32;] [lfplus_ccs_linearize:] a sharded context (a
 * transport or lfplus_set_sharding_model; a rank-sharded form is not built, as for lfplus_witness_from_z); no resident witness of 2^nvars ring elements,
 * nvars >= 1; rowptr NULL and resident matrices that do not number t (or of another n); a CSR array as lfplus_decompose refuses it.  [lfplus_ccs_check: after
 * the shape, the refusals of lfplus_r1cs_check.]  A NULL context is LFPLUS_E_ARG (without a device none can exist).
 *   lfplus_ccs_check is lfplus_r1cs_check for this shape: cm_f = A f (NULL: not checked), the norm rule absmax < bound, and the row-wise residual
 * sum_i c_i prod_{j in S_i} (M_j f)[row] = 0 in the ring, fused (the t product tables are never written; *first_bad = the smallest failing row, n when none fails),
 * reported as LFPLUS_REL_CCS.  Read-only; the context stays usable after every return.
 *   No _dev twins: the only O(n) input is the resident witness, which has lfplus_set_witness_dev / lfplus_witness_from_z_dev; everything these calls take or return is small.
 *   The prover object and the flat proof for these instances: lfplus_prover_create_ccs / lfplus_verify_ccs below.
 *   Not built: sharded contexts (and so a sharded CCS prover). */
typedef struct { uint32_t t, q; const uint32_t *S_off /* q + 1 */, *S_idx /* S_off[q] */; const uint64_t *c /* q x 16 canonical words */; } lfplus_ccs;
int lfplus_ccs_linearize(lfplus_ctx *ctx, lfplus_transcript *t, const lfplus_ccs *shape, const uint32_t *const *rowptr, const uint32_t *const *col,
                         const uint64_t *const *val /* t matrices; rowptr NULL: the resident ones, which must number t */, uint64_t *msgs, uint64_t *ro, uint64_t *evals);
int lfplus_ccs_verify(lfplus_transcript *t, uint32_t nvars, const lfplus_ccs *shape, const uint64_t *msgs, const uint64_t *evals, uint64_t *ro, int *stage);
int lfplus_ccs_check(lfplus_ctx *ctx, const uint64_t *cm_f, const lfplus_ccs *shape, const uint32_t *const *rowptr, const uint32_t *const *col,
                     const uint64_t *const *val, uint64_t bound, unsigned *failed, uint64_t *first_bad, uint64_t *absmax);

/* ---- PlusProver / PlusVerifier for committed CCS instances: the objects above with "the linearization of this prover" a CCS shape in place of ComR1CS.  One
 * body serves both (lfp_prover.cpp): lfplus_ccs_linearize per fresh instance as it arrives (from_f on the second stream, as for R1CS), lfplus_mlin and
 * lfplus_decompose_resident with nM = t.  SELF-CONSISTENT, PINNED AT THE R1CS SHAPE: with t = 3, S = ({0,1},{2}), c = (1, -1) every field word after the header,
 * the accumulator and the transcript state are those of the lfplus_prover_create prover on the same inputs (through the general round kernel: the object has one
 * linearization path per kind, no dispatch on the shape).
 *   lfplus_prover_create_ccs is lfplus_prover_create with the shape in place of nM (rowptr / col / val name shape->t matrices).  The shape is COPIED (S_off, S_idx,
 * c are free again on return); its refusals are those of lfplus_ccs_linearize, in that order, LFPLUS_E_ARG with *out = NULL before any context is created.  The
 * result is an ordinary lfplus_prover: ingest, set_instances, their _dev twins, prove, accumulator(_dev), decide, wait_stream, destroy and last_error work on it
 * unchanged, with the same state machine and failed-state rules; prove and decide expect the CCS layout below.  Unsharded only.
 *   The flat proof: the layout above with another header and per fresh instance i < nfresh (d = max |S_i|)
 *     msgs        nvars * (d + 2) * 16     r        nvars          evals    (1 + t) * 16
 *   then the CmProof, LinB2X and DecompProof fields with nM = t; lfplus_proof_fields(nfresh) fields as before.
 *   header        LFPLUS_PROOF_MAGIC_CCS, L, nfresh, nvars, k, l, kappa, t, q, d, S_off[q], 0      (LFPLUS_PROOF_HEADER_CCS words; CHECKED, never used for sizing)
 * lfplus_proof_len_ccs / lfplus_proof_layout_ccs: as their namesakes; a shape lfplus_ccs_linearize refuses, or parameters outside the envelope above, give
 * 0 / LFPLUS_E_ARG.
 *   lfplus_verify_ccs is lfplus_verify for this layout, host only (no context, no GPU): a refused shape, a length or header that differs from the verifier's own
 * statement, or a NULL proof is LFPLUS_E_ARG before any word of a field is read and with the transcript untouched; then lfplus_ccs_verify per fresh instance,
 * lfplus_cm_verify (nM = t), lfplus_decomp_verify (1 + t).  *which / *stage are numbered exactly as in lfplus_verify (stage of a fresh instance: 1 = a sumcheck
 * round, 2 = the final identity -- evaluations of the LAST round that were changed show there, the sums of the earlier rounds having held). */
#define LFPLUS_PROOF_HEADER_CCS 12
#define LFPLUS_PROOF_MAGIC_CCS 0x4C46504C55533032ULL   /* the bytes "LFPLUS02", most significant first */
int lfplus_prover_create_ccs(int device, const lfplus_params *params, const uint64_t *A, uint64_t seed, uint64_t n, const lfplus_ccs *shape,
                             const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val, uint32_t ncomp, lfplus_transcript *transcript,
                             lfplus_prover **out);
uint64_t lfplus_proof_len_ccs(const lfplus_params *params, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh);
int lfplus_proof_layout_ccs(const lfplus_params *params, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh, uint64_t *offsets, uint64_t *lengths,
                            uint32_t nfields);
int lfplus_verify_ccs(const lfplus_params *params, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh, lfplus_transcript *transcript,
                      const uint64_t *proof, uint64_t proof_words, int *which, int *stage);
/* Is every fresh instance named by the last ingest / set_instances in its relation?  Asked where the instance lives, on the resident matrices: lfplus_ccs_check
 * for a prover of lfplus_prover_create_ccs, lfplus_r1cs_check for one of lfplus_prover_create (neither the linearization nor the prove checks satisfaction, as
 * the reference's do not).  Outputs are arrays of nfresh entries: ok[i] = 1 / 0, failed[i] = the LFPLUS_REL_* bits, first_bad[i] = the smallest failing row (n:
 * none), absmax[i]; cm_f is compared when set_instances supplied it, ||f||_inf < bound when bound != 0.  Valid between naming the instances and the prove
 * (LFPLUS_E_ARG otherwise, and on a FAILED prover).  Waits for the upload worker; an upload that failed fails the prover exactly as it would in the prove.
 * LFPLUS_OK when all hold, LFPLUS_E_REJECT when one does not (all outputs written in both cases).  Read-only: the transcript is untouched and the following
 * prove writes the proof it would have written without the call. */
int lfplus_prover_check_fresh(lfplus_prover *prover, uint64_t bound, int *ok, unsigned *failed, uint64_t *first_bad, uint64_t *absmax);

#ifdef __cplusplus
}
#endif
#endif
