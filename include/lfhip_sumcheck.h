/*
 * lfhip_sumcheck.h -- part of the C ABI of liblfhip.so (lfhip.h includes it; include lfhip.h, not this file): MLSumcheck over any sum of products of
 * multilinear extensions.  Same conventions as lfhip.h: host pointers unless marked, 0 or a negative LF_ERR_* code, nothing aborts.  LFHIP_ABI_VERSION is
 * unchanged: additions only.
 */
#ifndef LFHIP_SUMCHECK_H
#define LFHIP_SUMCHECK_H
#ifndef LFHIP_H
#error "include lfhip.h"
#endif

/* ---- MLSumcheck::prove_as_subprotocol / verify_as_subprotocol (utils/sumcheck.rs:53-104, utils/sumcheck/prover.rs:56-162, utils/sumcheck/verifier.rs:92-257)
 * for the VirtualPolynomial of utils/sumcheck/utils.rs:24-75: a (coefficient, indices) product list over a flat list of MLE tables,
 *      g(x) = sum_{i < nterms} coef_i * prod_{k in [term_off[i], term_off[i+1])} T_{term_idx[k]}(x),      x in {0,1}^nvars.
 * Tables are ntables x 2^nvars ring elements in NTT form (table j at tables + j * 2^nvars * lf_ring_words), GENERAL ring elements (they need not be
 * slot-constant); entry x of a table has variable 1 in bit 0 of x (DenseMultilinearExtension: the first round fixes the lowest bit).  Coefficients are ring
 * elements in NTT form.  A table may be used by several terms and several times in one term (a square).  All entry points work on a BARE context -- no CCS,
 * no Ajtai matrix -- and on both rings; the verifier needs no context at all.
 *   The state of this sumcheck is the context's own and is separate from lf_sumcheck_lin_* and lf_sumcheck_fold_*: the three may be interleaved on one
 * context.  lf_mlsumcheck_begin while a generic sumcheck is active replaces it (as lf_sumcheck_lin_begin does).
 *   Refusals of begin / prove, in this order: a NULL argument, a table index >= ntables, term_off that is not increasing (every term has at least one factor), a
 * coefficient word >= p -> LF_ERR_INVALID; anything outside the envelope stated on the fields below -> LF_ERR_UNSUPPORTED; a sharded context
 * (lf_set_sharding, lf_dist_init, lf_set_sharding_model) or one with an external basis installed (lf_set_ext_basis) -> LF_ERR_UNSUPPORTED: OUT OF SCOPE here,
 * the generic sumcheck runs on one GPU in the default basis; a table word >= p -> LF_ERR_INVALID (host tables are tested on the host before anything is
 * enqueued, device tables by the relayout kernel that reads them: the flag the kernel raises comes home before begin returns; either way this test comes
 * after the envelope, which says how many words there are); allocation failure -> LF_ERR_HIP.  Of the split form: lf_mlsumcheck_round before a begin, with
 * r_prev NULL in a later round or non-NULL in round 1, or after nvars rounds, and lf_mlsumcheck_final before the last round -> LF_ERR_STATE.
 *   After any refusal the context is usable and holds no half-installed sumcheck: a begin refused by its arguments leaves a sumcheck in progress as it was;
 * one refused after the tables were touched (a device word >= p, an allocation failure) leaves none, the next round is LF_ERR_STATE.  lf_mlsumcheck_prove
 * refuses everything above before the first absorb; the transcript is untouched then. */
typedef struct {
    uint32_t nvars;            /* m = 2^nvars entries per table, 1 <= nvars <= 30 */
    uint32_t ntables;          /* T, 1..16 */
    uint32_t nterms;           /* q, 1..16 */
    uint32_t degree;           /* the degree the prover absorbs and sends degree+1 evaluations for; max_i |S_i| <= degree <= 8 */
    const uint32_t *term_off;  /* q+1 offsets into term_idx; every term has 1..8 factors; term_off[q] <= 64 */
    const uint32_t *term_idx;  /* table indices < T; an index may repeat inside a term (a square) and across terms */
    const uint64_t *coef;      /* q ring elements, NTT form, any value including 0 */
} lf_vpoly;

/* The split form (the caller's transcript stays in charge between the rounds).  begin copies the descriptor and the coefficients and relays the tables into
 * buffers of the context: the caller's arrays are never written and are free again when the call returns. */
int lf_mlsumcheck_begin(lf_ctx *, const lf_vpoly *, const uint64_t *tables /* T x m ring elements */);
/* the same with `tables` in memory of the context's device, under every rule of the _dev calls of lfhip.h (pointer checks, canonical words, ordering by
 * lf_ctx_wait_stream); spelled _device as lf_ring_mul_device is */
int lf_mlsumcheck_begin_device(lf_ctx *, const lf_vpoly *, const uint64_t *tables /* dev: T x m ring elements */);
/* round i = 1 .. nvars: fixes the previous variable at r_prev (tau words; NULL in round 1), then evaluates the round polynomial at 0 .. degree */
int lf_mlsumcheck_round(lf_ctx *, const uint64_t *r_prev /* tau words, NULL in round 1 */, uint64_t *evals_out /* (degree+1) ring elements */);
/* valid after nvars rounds: fixes the last variable at r_last and returns every table's value at the whole point.  DEVIATION from ProverState
 * (sumcheck/prover.rs): the reference leaves the MLEs fixed nvars - 1 times and each caller evaluates them next; this call is that next step, done where the
 * tables already are */
int lf_mlsumcheck_final(lf_ctx *, const uint64_t *r_last /* tau words */, uint64_t *evals_out /* T ring elements */);
/* drops the state; always LF_OK (LF_ERR_INVALID for a NULL context) */
int lf_mlsumcheck_end(lf_ctx *);

/* prove_as_subprotocol in one call: absorb(nvars), absorb(degree), then per round absorb_slice(evaluations), get_challenge, absorb(challenge as a ring
 * element) -- the loop over the split form above.  msgs_out: nvars x (degree+1) ring elements (the Proof); point_out: the nvars challenges, tau words each;
 * final_out (may be NULL): the T table values at the point, as lf_mlsumcheck_final.  The transcript must be of the context's ring */
int lf_mlsumcheck_prove(lf_ctx *, lf_transcript *, const lf_vpoly *, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out, uint64_t *final_out);
int lf_mlsumcheck_prove_device(lf_ctx *, lf_transcript *, const lf_vpoly *, const uint64_t *tables /* dev */, uint64_t *msgs_out, uint64_t *point_out,
                               uint64_t *final_out);
/* verify_as_subprotocol on the host: no context, no GPU; the default ring tables of `ring`.  claimed_sum: one ring element; msgs: nvars x (degree+1) ring
 * elements; point_out: nvars x tau words; expected_out: one ring element, the subclaim's expected evaluation g(point).  LF_OK, or LF_ERR_REJECT with
 * expected_out[0] = the index (from 0) of the first round whose p(0) + p(1) is not the running claim; the transcript has then advanced over ALL rounds, as
 * the reference's has (the verifier absorbs every message before it checks, verifier.rs:92-139).  NULL argument, a transcript of the other ring, an
 * unknown ring, a word >= p in claimed_sum or msgs -> LF_ERR_INVALID; nvars == 0 or > 30, degree == 0 or > 8 -> LF_ERR_UNSUPPORTED */
int lf_mlsumcheck_verify(int ring, lf_transcript *, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum, const uint64_t *msgs, uint64_t *point_out,
                         uint64_t *expected_out);

#endif
