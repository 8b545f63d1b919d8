/*
 * lfhip_tables.h -- part of the C ABI of liblfhip.so (lfhip.h includes it; include lfhip.h, not this file): the protocol's own tables from a witness, on the
 * device.  Same conventions as lfhip.h: 0 or a negative LF_ERR_* code, nothing aborts.  LFHIP_ABI_VERSION is unchanged: additions only.
 */
#ifndef LFHIP_TABLES_H
#define LFHIP_TABLES_H
#ifndef LFHIP_H
#error "include lfhip.h"
#endif

/* ---- witness tables: f-hat, z, M z, M^T v and fix_variables on tables ---------------------------------------------------------------------------------
 * What lf_sumcheck_fold_begin(_dev), lf_sumcheck_lin_begin(_dev) and lf_mlsumcheck_*(_device) take as tables, built from a witness handle without leaving the
 * GPU: the f-hat multilinear extensions (Witness::get_fhat, arith.rs:273-297), z = x || 1 || w_ccs (arith.rs:399-409), the M_j z tables (calculate_Mz_mles,
 * utils/mle_helpers.rs:137-146), the transposed product M_j^T v for a general vector v, and DenseMultilinearExtension::fix_variables on whole tables.  Both
 * rings, every base and envelope lf_ccs_load accepted (small bases and wide CCS included: nothing here depends on b).
 *   Each call has a twin ending in _device whose O(n) arrays are the caller's own memory on the context's device: everything lfhip.h says under
 * "device-resident callers" holds (AoS canonical words, the pointer check, ordering through lf_ctx_wait_stream, results complete on return).  x (the public
 * input, l ring elements) and the points are host memory in both spellings.  Every array but x is in NTT form; on a context in an external basis
 * (lf_set_ext_basis) arrays, x and points are read and written in external coordinates like those of every other call.
 *   f-hat layout: write f_coeff for the N x d canonical coefficient words of the witness (lf_witness_get_f_coeff).  Entry i < N of table j < tau is the ring
 * element whose slot k < 8 is the base-field constant f_coeff[i][8 j + k] -- word k tau of the element holds it, the other words of the slot are 0 -- and
 * entries N <= i < m are zero.  (A constant slot is the same words in any basis.)
 *   Refusals, in this order: a NULL argument, a handle of another context or with another N than the loaded system's -> LF_ERR_INVALID; no CCS loaded (every
 * call but lf_mle_fix_variables, which works on a bare context) -> LF_ERR_STATE; j >= t, count == 0, len not a power of two, nfix outside 1 .. log2(len), a
 * word of x, of a point or of a host array that is not below the modulus -> LF_ERR_INVALID; a sharded context (transport, RCCL or sharding model: a rank holds slices) ->
 * LF_ERR_UNSUPPORTED; a _device pointer that is not device memory of the context's device, or an input range that overlaps `out` -> LF_ERR_INVALID, nothing
 * launched; allocation failure -> LF_ERR_HIP.  A word of a DEVICE array that is not below the modulus is found by the kernel that reads it: LF_ERR_INVALID.
 * After any refusal a _device output is untouched and the context is usable. */
/* Witness::get_fhat for `count` witnesses: out = count * tau tables of m = 2^s ring elements, table (w tau + j) = f-hat_j of wits[w]; contiguous, in the order
 * lf_sumcheck_fold_begin takes them from slot 5 on */
int lf_witness_get_fhat(lf_ctx *, const lf_witness *const *wits, unsigned count, uint64_t *out);
int lf_witness_get_fhat_device(lf_ctx *, const lf_witness *const *wits, unsigned count, uint64_t *out /* dev */);
/* z = x || 1 || w_ccs: n = l + 1 + wit_len ring elements */
int lf_witness_get_z(lf_ctx *, const lf_witness *, const uint64_t *x, uint64_t *out);
int lf_witness_get_z_device(lf_ctx *, const lf_witness *, const uint64_t *x /* host */, uint64_t *out /* dev */);
/* calculate_Mz_mles: out = t tables of m ring elements, table j = M_j z, z as above */
int lf_witness_mz(lf_ctx *, const lf_witness *, const uint64_t *x, uint64_t *out);
int lf_witness_mz_device(lf_ctx *, const lf_witness *, const uint64_t *x /* host */, uint64_t *out /* dev */);
/* out (n ring elements) = M_j^T v: out[c] = sum over the entries (r, c) of M_j of M_j[r][c] (.) v[r], slot-wise; v = m GENERAL ring elements (not only
 * slot-constant ones).  The words of out do not depend on how many entries a column has (columns of many entries take a path of their own). */
int lf_spmv_t(lf_ctx *, unsigned j, const uint64_t *v, uint64_t *out);
int lf_spmv_t_device(lf_ctx *, unsigned j, const uint64_t *v /* dev: m */, uint64_t *out /* dev: n */);
/* DenseMultilinearExtension::fix_variables on tables: fixes the LOWEST nfix variables (the order of the sumcheck rounds) at point[0..nfix) (tau words each,
 * host); out = ntables tables of len >> nfix ring elements.  len = 2^nv, 1 <= nfix <= nv; nfix == nv leaves what lf_mle_eval_batch returns. */
int lf_mle_fix_variables(lf_ctx *, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nfix, uint64_t *out);
int lf_mle_fix_variables_device(lf_ctx *, const uint64_t *tables /* dev */, size_t ntables, size_t len, const uint64_t *point, unsigned nfix,
                                uint64_t *out /* dev */);

#endif
