// bb_capi.h -- BabyBearRingNTT backend behind the C ABI (include/lfhip.h).  lf_capi.cpp forwards the entry points that are
// really this backend's own to the matching BbCtx method; the ring-generic ones go to the shared bodies of lf_ring_host.h.  Same flat layouts as the
// Goldilocks backend with ring elements of 72 words and tau = 9.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lfhip.h"
#include "bb_host.h"

struct lf_witness;
namespace lfdist { struct Comm; }

namespace lfbb {

struct BbCtxImpl;

struct BbCtx {
    BbCtxImpl *p;
    static int create(BbCtx **out, lf_ctx *owner, int device);
    void destroy();

    int set_sharding(int rank, int world, lf_exchange_fn cb, void *user);
    int dist_init(int rank, int world, const uint8_t *id128);
    lfdist::Comm *comm();
    void set_digit_mode(int mode);
    bool have_ccs() const;
    const lf_params &params() const;
    size_t dim_n() const;
    size_t dim_m() const;
    size_t dim_N() const;
    uint32_t kappa() const;
    int set_ring_tables(uint64_t nonres, const uint64_t *y);
    int get_ring_tables(uint64_t *nonres, uint64_t *y);
    int synchronize();
    int mem_info(size_t *free_bytes, size_t *total_bytes);
    int selftest_field(uint64_t seed, uint32_t n, uint64_t *mismatches);
    int ajtai_load(const uint64_t *A, size_t kappa, size_t n);
    int ajtai_generate(uint64_t seed, size_t kappa, size_t n);
    int ajtai_commit(const uint64_t *f, size_t n, size_t batch, uint64_t *out);
    // commit_coeff / decompose_and_commit_{coeff,ntt}: element i of f [batch][count] -> its balanced base-2^lb digits, columns [i L, (i + 1) L) (lb 0, L 1: itself)
    int ajtai_commit_gadget(const uint64_t *f, bool ntt_in, size_t count, uint32_t lb, unsigned L, size_t batch, uint64_t *out);
    int ccs_load(const lf_params *p, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val,
                 const uint32_t *S_off, const uint32_t *S_idx, const uint64_t *cc);
    int sumcheck_lin_begin(const uint64_t *tables, const uint64_t *eq_point);
    int sumcheck_lin_round(const uint64_t *r_prev, uint64_t *evals_out);
    int sumcheck_lin_end();
    int sumcheck_fold_begin(const uint64_t *tables, const uint64_t *mu);
    int sumcheck_fold_round(const uint64_t *r_prev, uint64_t *evals_out);
    int sumcheck_fold_end();
    int linearize(BbTranscript &tr, const uint64_t *cccs, const lf_witness *wit, uint64_t *lcccs_out, uint64_t *lin_proof_out);
    int fold_step(BbTranscript &tr, const uint64_t *acc, const lf_witness *w_acc, const uint64_t *cm_i, const lf_witness *w_i,
                  uint64_t *lcccs_out, lf_witness **w_out, uint64_t *proof);
    int decomposition_prove(BbTranscript &tr, const uint64_t *lcccs, const lf_witness *wit, uint64_t *lcccs_s_out, uint64_t *dec_proof_out);
    int folding_prove(BbTranscript &tr, const uint64_t *lcccs_s, const lf_witness *w_left, const lf_witness *w_right, uint64_t *lcccs_out,
                      lf_witness **w_out, uint64_t *fold_proof_out);
    int last_phase_ms(float *out);
    int last_kernel_stats(float *fold_ms, int *fold_n, float *aj_ms, int *aj_n);
    unsigned fold_split_rounds() const;   // table rounds of the last folding sumcheck that ran in the split eq form
    unsigned fold_paths() const;   // rounds of the last folding sumcheck that ran as int8 GEMMs (bit i-1 = round i)
};

int bb_verify_host(const lf_params *p, const uint32_t *S_off, const uint32_t *S_idx, const uint64_t *c, BbTranscript &tr, const uint64_t *acc,
                   const uint64_t *cm_i, const uint64_t *proof, uint64_t *lcccs_out, int *failed_stage);

}  // namespace lfbb
