/*
 * lfhip_prover.h -- part of the C ABI of liblfhip.so (lfhip.h includes it; include lfhip.h, not this file): the chained NIFS prover as an object.
 * Same conventions as lfhip.h: host pointers unless marked, 0 or a negative LF_ERR_* code, nothing aborts.  LFHIP_ABI_VERSION is unchanged: additions only
 * (a binding asks for a symbol it needs).
 */
#ifndef LFHIP_PROVER_H
#define LFHIP_PROVER_H
#ifndef LFHIP_H
#error "include lfhip.h"
#endif

/* ---- lf_prover: an IVC-style chain (nifs/tests.rs:58-117, examples/e2e.rs made a loop) ------------------------------------------------------------------
 * Every step ingests a new witness of the context's constraint system, commits it and folds it into an accumulator (LCCCS + folded witness) that the object
 * owns on the device.  The prover BORROWS an lf_ctx with a constraint system loaded and an Ajtai matrix resident -- either ring, any envelope the context
 * accepted (wide CCS, b = 4 / 8 / 16, l > 1, an external basis) -- and is host code over the entry points of lfhip.h: every output is word for word what
 * the sequence lf_witness_from_w_ccs(_begin) -> lf_witness_commit -> lf_fold_step produces, with the lengths of lf_lcccs_len_ring, lf_cccs_len_ring and
 * lf_proof_len_ring; `failed` / `first_bad` are those of lf_cccs_check / lf_lcccs_check; the _dev pointers follow the rules of "device-resident callers" in
 * lfhip.h; in an external basis (lf_set_ext_basis) inputs and outputs are in the caller's basis, as for the calls underneath.
 *
 * State machine: EMPTY -> READY (init / resume) -> READY+PENDING (ingest) -> READY (prove).
 *   prove, decide, accumulator, ingest or check_fresh in EMPTY; a second ingest while one is pending; prove or check_fresh without a pending instance; init or
 * resume on a READY prover: LF_ERR_STATE.  NULL arguments: LF_ERR_INVALID (a transcript of the other ring too).  lf_prover_create: a context without CCS or
 * matrix is LF_ERR_STATE, a sharded one (world > 1: a transport or lf_set_sharding_model) LF_ERR_UNSUPPORTED.  The prover records the context's lf_params, N
 * and kappa at create and compares them at every call: a context whose CCS or matrix was loaded again since returns LF_ERR_STATE and nothing is touched.
 * One thread per prover at a time; destroy the provers before their context.
 *   Failures: an error before the transcript is advanced (a failed ingest job, a failed commit, any refusal of ingest / check_fresh / prove above but that of
 * a replaced context) drops the pending instance -- its w_ccs is no longer borrowed --, keeps the accumulator and leaves the prover usable.  An error inside lf_linearize or lf_fold_step makes the prover FAILED: every later call except destroy and
 * last_error returns LF_ERR_STATE with a message.  No C++ exception leaves the library.
 *   Memory: the old accumulator witness and the consumed fresh witness are freed by the prove that replaces them; their planes go back to the recycle pool the
 * next ingest draws from, so a chain in steady state allocates and frees no device memory.
 *   The fresh witness is committed (Witness::commit) at the head of the prove, on the context's main lane, with or without LF_PROVER_COMMIT_INLINE: the flag
 * names the one placement there is.  Committing inside the ingest job was measured slower and removed ("The prover object").
 *   Overlap: the ingest job runs next to whatever the caller does between lf_prover_ingest and the next call that needs the witness.  In a loop that does nothing
 * in between, the ingestion is not hidden behind a fold step as in the call-level sequence (which may begin it before lf_fold_step): 1.6 ms of an 18 ms step at
 * 2^20 rows. */
typedef struct lf_prover lf_prover;
enum { LF_PROVER_COMMIT_INLINE = 1 };   /* flags: commit the fresh witness at the head of prove on the main lane, never inside the ingest job */
int lf_prover_create(lf_ctx *, unsigned flags, lf_prover **out);   /* any other flag bit: LF_ERR_INVALID */
void lf_prover_destroy(lf_prover *);                               /* NULL ok; abandons a pending job, frees the accumulator and the fresh witness, never touches the context */
const char *lf_prover_last_error(const lf_prover *);               /* never NULL, also for a NULL prover; "" after a call that succeeded */
/* first accumulator = linearization of (x_ccs, w_ccs): from_w_ccs + Witness::commit + lf_linearize on `t` (what every chain of the tests does) */
int lf_prover_init(lf_prover *, lf_transcript *t, const uint64_t *w_ccs, const uint64_t *x_ccs /* l */, uint64_t *lcccs_out, uint64_t *lin_proof_out);
/* or: take up a chain again from (LCCCS, folded witness f in NTT form, N elements) */
int lf_prover_resume(lf_prover *, const uint64_t *lcccs, const uint64_t *f_ntt);
int lf_prover_resume_dev(lf_prover *, const uint64_t *lcccs, const uint64_t *f_ntt_dev);
/* names the fresh instance of the NEXT prove and returns at once (lf_witness_from_w_ccs_begin); w_ccs is borrowed until that prove (or destroy) returns,
 * x_ccs (l elements) is copied */
int lf_prover_ingest(lf_prover *, const uint64_t *w_ccs, const uint64_t *x_ccs);
int lf_prover_ingest_dev(lf_prover *, const uint64_t *w_ccs_dev, const uint64_t *x_ccs);   /* blocking, as lf_witness_from_w_ccs_dev; not borrowed afterwards */
/* R_CCCS of the pending instance where it lives (joins the job; the commitment it computes is kept for the prove): lf_cccs_check of (cm || x_ccs, witness)
 * with the commitment the prover computed itself, so LF_REL_CM cannot be raised here.  LF_ERR_REJECT keeps the pending instance; any other error drops it */
int lf_prover_check_fresh(lf_prover *, uint64_t bound, unsigned *failed, uint64_t *first_bad);
/* NIFSProver::prove of (accumulator, pending instance) on `t`; the folded pair becomes the accumulator, what it replaces is freed.
 * cccs_out (cm || x_ccs, may be NULL) is the fresh CCCS a verifier needs next to the proof */
int lf_prover_prove(lf_prover *, lf_transcript *t, uint64_t *cccs_out, uint64_t *lcccs_out, uint64_t *proof_out);
int lf_prover_accumulator(lf_prover *, uint64_t *lcccs_out, uint64_t *f_ntt_out);           /* either may be NULL */
int lf_prover_accumulator_dev(lf_prover *, uint64_t *lcccs_out, uint64_t *f_ntt_dev_out);
int lf_prover_decide(lf_prover *, uint64_t bound, unsigned *failed);                        /* lf_lcccs_check of the accumulator; read-only */
uint64_t lf_prover_steps(const lf_prover *);                                                /* proves since init / resume; 0 for a NULL prover */

#endif
