/*
 * lfhip_parts.h -- part of the C ABI of liblfhip.so (lfhip.h includes it; include lfhip.h, not this file): the decomposed witnesses as handles.
 * Same conventions as lfhip.h: host pointers, 0 or a negative LF_ERR_* code, nothing aborts.  LFHIP_ABI_VERSION is unchanged: additions only.
 */
#ifndef LFHIP_PARTS_H
#define LFHIP_PARTS_H
#ifndef LFHIP_H
#error "include lfhip.h"
#endif

/* ---- decomposed witnesses: the wit_s LFDecompositionProver::prove returns and the w_s LFFoldingProver::prove consumes, as handles ---------------------
 * A part handle is an ordinary witness of the context with planes of its own: the getters (and their _dev twins), lf_witness_commit, lf_lcccs_check and
 * lf_witness_free work on it, and each part is freed alone.  Both rings, every base lf_ccs_load accepted, both digit rules, sharded contexts included
 * (witnesses are replicated; the work is local).
 *   Refusals, in this order: a NULL argument, a handle of another context -> LF_ERR_INVALID; no CCS loaded -> LF_ERR_STATE; count != P.K (2 P.K for
 * lf_folding_prove_parts), a handle with another N -> LF_ERR_INVALID; K digits that do not cover B/2 under the active digit rule (lf_set_digit_mode after the
 * load) -> LF_ERR_UNSUPPORTED, the test lf_decomposition_prove performs where a step starts.  lf_witness_recompose and lf_folding_prove_parts then look at the
 * digits, on the device: one outside the rule's range (-b/2 <= d <= b/2 under rule 0, -b/2 <= d < b/2 under rule 1 at b > 2), or legal digits that are not
 * the decomposition of their own sum (a tie written (-b/2, +1) for (+b/2, 0), a non-zero last carry) -> LF_ERR_INVALID; a sum lf_witness_from_f_coeff would
 * refuse -> that call's code (LF_ERR_NORM, or LF_ERR_UNSUPPORTED for +2^31 at B = 2^32).  Allocation failure -> LF_ERR_HIP.
 *   After any error every output handle is NULL, nothing made inside the call is left allocated, the transcript has absorbed nothing and the context is
 * usable: all these refusals come before the first absorb (lf_decomposition_prove_parts cuts the parts first and frees them if the prover then fails).
 *   DEVIATION from the reference: LFFoldingProver::prove accepts any 2K witnesses.  lf_folding_prove_parts accepts those that are the decomposition of their
 * sum -- all LFDecompositionProver ever produces -- because the fold step cuts the parts again from the sum; anything else is a loud LF_ERR_INVALID, never a
 * proof about other witnesses.  mz_mles (K t m ring elements) is not returned: the folding prover rebuilds M z on the device. */
/* decompose_witness (nifs/decomposition.rs:162-167): parts_out[k], k < P.K, = Witness::from_f_coeff(part k of
 * decompose_B_vec_into_k_vec(wit.f_coeff)) under the context's digit rule; K fresh handles of this context. */
int lf_witness_decompose(lf_ctx *, const lf_witness *wit, lf_witness **parts_out /* P.K */);
/* the inverse: *out = the witness whose base-b parts are parts[0..count), count == P.K */
int lf_witness_recompose(lf_ctx *, const lf_witness *const *parts, unsigned count, lf_witness **out);
/* LFDecompositionProver::prove with its wit_s: lf_decomposition_prove + the K part handles */
int lf_decomposition_prove_parts(lf_ctx *, lf_transcript *, const uint64_t *lcccs, const lf_witness *wit,
                                 uint64_t *lcccs_s_out, uint64_t *dec_proof_out, lf_witness **parts_out /* P.K */);
/* LFFoldingProver::prove with the reference's w_s: 2K witnesses (K of the accumulator, then K of the fresh instance), recomposed on the device; outputs and
 * transcript state are word for word those of lf_folding_prove on the two sums */
int lf_folding_prove_parts(lf_ctx *, lf_transcript *, const uint64_t *lcccs_s, const lf_witness *const *w_s, unsigned count /* 2 P.K */,
                           uint64_t *lcccs_out, lf_witness **w_out, uint64_t *fold_proof_out);

#endif
