// bb_capi.h -- BabyBearRingNTT backend behind the C ABI (include/lfhip.h).  lf_capi.cpp forwards the entry points that are
// really this backend's own to the matching BbCtx method; the ring-generic ones go to the shared bodies of lf_ring_host.h.  Same flat layouts as the
// Goldilocks backend with ring elements of 72 words and tau = 9.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lfhip.h"
#include "bb_host.h"

struct lf_witness;
struct CtxCoreBase;
namespace lfdist { struct Comm; }

namespace lfbb {

struct BbCtxImpl;

struct BbCtx {
    BbCtxImpl *p;
    static int create(BbCtx **out, lf_ctx *owner, int device);
    CtxCoreBase &core();   // what the context shares with the Goldilocks one (lf_ctx_core.h): the read-outs and the external-basis marshalling need no more
    void destroy();

    int set_sharding(int rank, int world, lf_exchange_fn cb, void *user);
    int dist_init(int rank, int world, const uint8_t *id128);
    int set_ring_tables(uint64_t nonres, const uint64_t *y);
    int get_ring_tables(uint64_t *nonres, uint64_t *y);
    int selftest_field(uint64_t seed, uint32_t n, uint64_t *mismatches);
    int linearize(BbTranscript &tr, const uint64_t *cccs, const lf_witness *wit, uint64_t *lcccs_out, uint64_t *lin_proof_out);
    int fold_step(BbTranscript &tr, const uint64_t *acc, const lf_witness *w_acc, const uint64_t *cm_i, const lf_witness *w_i,
                  uint64_t *lcccs_out, lf_witness **w_out, uint64_t *proof);
    int decomposition_prove(BbTranscript &tr, const uint64_t *lcccs, const lf_witness *wit, uint64_t *lcccs_s_out, uint64_t *dec_proof_out);
    int folding_prove(BbTranscript &tr, const uint64_t *lcccs_s, const lf_witness *w_left, const lf_witness *w_right, uint64_t *lcccs_out,
                      lf_witness **w_out, uint64_t *fold_proof_out);
};

int ccs_envelope(const lf_params *p);   // the limits of lf_ccs_load on this ring: LF_OK or LF_ERR_UNSUPPORTED
// lf_mlsumcheck_verify on this ring (lf_capi.cpp checked the arguments)
int bb_mlsumcheck_verify(BbTranscript &tr, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum, const uint64_t *msgs, uint64_t *point_out,
                         uint64_t *expected_out);
int bb_verify_host(const lf_params *p, const uint32_t *S_off, const uint32_t *S_idx, const uint64_t *c, BbTranscript &tr, const uint64_t *acc,
                   const uint64_t *cm_i, const uint64_t *proof, uint64_t *lcccs_out, int *failed_stage);

}  // namespace lfbb
