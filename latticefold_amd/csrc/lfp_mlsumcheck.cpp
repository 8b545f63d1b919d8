// lfp_mlsumcheck.cpp -- host driver of lfplus_mlsumcheck_* (include/lfplus.h): MLSumcheck::prove_as_subprotocol (latticefold utils/sumcheck.rs:53-80,
// sumcheck/prover.rs:56-162) over any sum of products of MLE tables on the Frog ring.  Kernels: lfp_mlsumcheck.hip.  The verifier is host code next to the other
// verifiers (lfp_protocol.cpp: lfplus_mlsumcheck_verify).
//   Rounds.  Round 1 reads the tables as they were handed over.  fix_variables of round i is deferred into the kernel of round i + 1 (k_mls_round<true>), which
// stores the fixed tables to one of two scratch buffers of the state (m / 2 and m / 4 entries per table; they alternate).  After the last round the stored tables
// hold two entries each and lfplus_mlsumcheck_final fixes the last variable.  Block partials are added on the device (k_sum_parts) and come home through the
// state's own pinned buffer: one stream synchronisation per round.
//   Tables.  Host tables are uploaded into a scratch buffer of the state.  Device tables of lfplus_mlsumcheck_prove_device are read IN PLACE by rounds 1 and 2 (the
// call returns after its last round, so the caller's array is free again on return); lfplus_mlsumcheck_begin_device copies them with the kernel that tests their
// words (k_copy_checked) -- the split form returns between the rounds, and a device-memory call leaves its inputs free for reuse when it returns.
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include "lfp_ctx.h"
#include "lfp_guard.h"
#include "lf_dev_ptr.h"

using lfdev::Origin;

struct LfpMls {
    u32 nvars = 0, T = 0, degree = 0;
    lfp::MlsDesc d;
    u32 done = 0;                      // rounds answered
    u32 cap = 2048;                    // workgroups of a round at most (LFPLUS_MLS_BLOCKS, read when the sumcheck begins)
    u64 *tab = nullptr;                // the uploaded / copied tables (nullptr: the caller's device array is read in place)
    u64 *fx[2] = {nullptr, nullptr};   // the fixed tables of round 2 onwards
    u64 *coef = nullptr, *part = nullptr, *res = nullptr;
    u32 *flag = nullptr;
    u64 *hres = nullptr;               // pinned: a round's (degree + 1) x 16 words / the T x 16 final values
    const u64 *cur = nullptr;          // the tables the next kernel reads, cur_len entries per table
    size_t cur_len = 0;
    int w = 0;                         // which of fx[] the next fused round writes
};

namespace {
constexpr u64 P = lfp::P;
u64 to_mont(u64 a) { return (u64)((((unsigned __int128)a) << 64) % P); }
void mls_free(lfplus_ctx *c, LfpMls *s) {
    if (!s) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    for (void *p : {(void *)s->tab, (void *)s->fx[0], (void *)s->fx[1], (void *)s->coef, (void *)s->part, (void *)s->res, (void *)s->flag}) c->own_free(p);
    if (s->hres) (void)hipHostFree(s->hres);
    delete s;
}
u32 block_cap() {
    const char *e = getenv("LFPLUS_MLS_BLOCKS");   // workgroups of a generic sumcheck round at most (default 2048, as cm_round_blocks); read once per sumcheck, by its begin
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= 65535 ? (u32)v : 2048u;
}
// the refusals of begin / prove in the order lfplus.h states them, up to the sharded context; on LFPLUS_OK `d` is the device descriptor
int validate(lfplus_ctx *c, const lfplus_vpoly *vp, const uint64_t *tables, const char *who, lfp::MlsDesc &d) {
    const std::string w(who);
    if (!vp || !tables || !vp->term_off || !vp->term_idx || !vp->coef) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    const u32 qs = vp->nterms < 16 ? vp->nterms : 16;      // (the envelope comes later: nothing beyond 16 terms / 64 factors is read before it holds)
    u32 lim = 0;
    for (u32 i = 0; i < qs; i++)
        if (vp->term_off[i + 1] > lim && vp->term_off[i + 1] <= 64) lim = vp->term_off[i + 1];
    for (u32 k = 0; k < lim; k++)
        if (vp->term_idx[k] >= vp->ntables) return fail(c, LFPLUS_E_ARG, w + ": table index " + std::to_string(vp->term_idx[k]) + " >= ntables");
    if (qs && vp->term_off[0] != 0) return fail(c, LFPLUS_E_ARG, w + ": term_off must start at 0");
    for (u32 i = 0; i < qs; i++)
        if (vp->term_off[i + 1] <= vp->term_off[i]) return fail(c, LFPLUS_E_ARG, w + ": term_off is not strictly increasing (every term has at least one factor)");
    if (!canonical(vp->coef, (size_t)qs * 16)) return fail(c, LFPLUS_E_ARG, w + ": non-canonical coefficient word");
    if (vp->nvars < 1 || vp->nvars > 28 || vp->ntables < 1 || vp->ntables > 16 || vp->nterms < 1 || vp->nterms > 16 || vp->degree < 1 || vp->degree > 8 ||
        vp->term_off[vp->nterms] > 64)
        return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= nvars <= 28, 1 <= ntables, nterms <= 16, 1 <= degree <= 8, at most 64 factors)");
    for (u32 i = 0; i < vp->nterms; i++) {
        const u32 nf = vp->term_off[i + 1] - vp->term_off[i];
        if (nf > 8 || nf > vp->degree) return fail(c, LFPLUS_E_ARG, w + ": a term has more than 8 factors, or more than `degree`");
    }
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported (the generic sumcheck runs on one GPU)");
    memset(&d, 0, sizeof(d));
    d.nt = vp->ntables; d.nterms = vp->nterms; d.degree = vp->degree;
    for (u32 i = 0; i <= vp->nterms; i++) d.off[i] = (uint8_t)vp->term_off[i];
    for (u32 k = 0; k < vp->term_off[vp->nterms]; k++) d.idx[k] = (uint8_t)vp->term_idx[k];
    for (u32 i = 0; i < vp->nterms; i++) {
        const u64 *cw = vp->coef + (size_t)i * 16;
        bool tail0 = true;
        for (int j = 1; j < 16; j++) tail0 = tail0 && cw[j] == 0;
        d.cls[i] = (uint8_t)(tail0 && cw[0] == 0 ? lfp::MLS_ZERO : tail0 && cw[0] == 1 ? lfp::MLS_ONE : tail0 && cw[0] == P - 1 ? lfp::MLS_MINUS_ONE : lfp::MLS_GENERAL);
    }
    return LFPLUS_OK;
}
// installs the sumcheck: everything validate() cannot see (the pointer of a device array, the words of the tables), then the state.  in_place: device tables
// stay where they are (the one-call prove)
int begin_impl(lfplus_ctx *c, const lfplus_vpoly *vp, const uint64_t *tables, Origin o, bool in_place, const char *who) {
    lfp::MlsDesc d;
    int rc = validate(c, vp, tables, who, d);
    if (rc) return rc;
    const bool dev = o == Origin::device;
    const size_t m = (size_t)1 << vp->nvars, T = vp->ntables, words = T * m * 16;
    if (dev && lfp_dev_ptr_check(c, tables, (uint64_t)T * m, who)) return LFPLUS_E_ARG;
    if (!dev && !canonical(tables, words)) return fail(c, LFPLUS_E_ARG, std::string(who) + ": non-canonical table word");
    HIPCHK(c, hipSetDevice(c->device));
    // from here on the tables are touched: the sumcheck in progress, if any, is gone whatever happens
    lfp_mls_drop(c);
    LfpMls *s = new LfpMls;
    s->nvars = vp->nvars; s->T = vp->ntables; s->degree = vp->degree; s->d = d;
    s->cap = block_cap();
    const u32 np = vp->degree + 1, nb0 = lfp::mls_round_blocks(m / 2, s->cap);
    const size_t resw = (size_t)(np > T ? np : T) * 16;
    bool ok = c->own_alloc(&s->coef, (size_t)vp->nterms * 16 * 8) == hipSuccess && c->own_alloc(&s->part, (size_t)nb0 * np * 16 * 8) == hipSuccess &&
              c->own_alloc(&s->res, resw * 8) == hipSuccess && c->own_alloc(&s->flag, 8) == hipSuccess &&
              hipHostMalloc((void **)&s->hres, resw * 8, hipHostMallocDefault) == hipSuccess;
    if (ok && (!dev || !in_place)) ok = c->own_alloc(&s->tab, words * 8) == hipSuccess;
    if (ok && vp->nvars >= 2) ok = c->own_alloc(&s->fx[0], words / 2 * 8) == hipSuccess;
    if (ok && vp->nvars >= 3) ok = c->own_alloc(&s->fx[1], words / 4 * 8) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        mls_free(c, s);
        return fail(c, LFPLUS_E_HIP, std::string(who) + ": out of memory (tables of the sumcheck)");
    }
    hipError_t e = hipMemcpyAsync(s->coef, vp->coef, (size_t)vp->nterms * 16 * 8, hipMemcpyHostToDevice, c->st);
    u32 flag = 0;
    if (e == hipSuccess && !dev) e = hipMemcpyAsync(s->tab, tables, words * 8, hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess && dev) {
        e = hipMemsetAsync(s->flag, 0, 4, c->st);
        if (e == hipSuccess) {
            if (in_place) lfp::launch_check_canonical(tables, words, s->flag, 1u, c->st);
            else lfp::launch_copy_checked(tables, s->tab, words, s->flag, 1u, c->st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, s->flag, 4, hipMemcpyDeviceToHost, c->st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) {
        mls_free(c, s);
        return fail(c, LFPLUS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    if (flag) {
        mls_free(c, s);
        return fail(c, LFPLUS_E_ARG, std::string(who) + ": non-canonical table word");
    }
    s->cur = s->tab ? s->tab : tables;
    s->cur_len = m;
    c->mls = s;
    return LFPLUS_OK;
}
int round_impl(lfplus_ctx *c, const uint64_t *r_prev, uint64_t *evals_out) {
    LfpMls *s = c->mls;
    if (!s) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_round: no sumcheck in progress (lfplus_mlsumcheck_begin)");
    if (!evals_out) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_round: null argument");
    if (s->done >= s->nvars) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_round: all " + std::to_string(s->nvars) + " rounds are answered (lfplus_mlsumcheck_final is next)");
    if (s->done == 0 && r_prev) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_round: round 1 takes no challenge (r_prev must be NULL)");
    if (s->done > 0 && !r_prev) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_round: r_prev is NULL in a later round");
    if (r_prev && *r_prev >= P) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_round: non-canonical challenge");
    HIPCHK(c, hipSetDevice(c->device));
    const u32 np = s->degree + 1;
    u32 nb;
    if (s->done == 0) {
        nb = lfp::mls_round_blocks(s->cur_len / 2, s->cap);
        lfp::launch_mls_round(s->cur, s->cur_len, s->cur_len / 2, s->d, s->coef, nb, s->part, c->st);
    } else {      // the previous tables, fixed at r_prev on the way in and stored
        const size_t half = s->cur_len / 4, ldo = s->cur_len / 2;
        u64 *outp = s->fx[s->w];
        nb = lfp::mls_round_blocks(half, s->cap);
        lfp::launch_mls_round_fused(s->cur, s->cur_len, half, s->d, s->coef, to_mont(*r_prev), outp, ldo, nb, s->part, c->st);
        s->cur = outp; s->cur_len = ldo; s->w ^= 1;
    }
    lfp::launch_sum_parts(s->part, nb, (size_t)np * 16, np * 16, s->res, c->st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s->hres, s->res, (size_t)np * 16 * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    memcpy(evals_out, s->hres, (size_t)np * 16 * 8);
    s->done++;
    return LFPLUS_OK;
}
int final_impl(lfplus_ctx *c, const uint64_t *r_last, uint64_t *evals_out) {
    LfpMls *s = c->mls;
    if (!s) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_final: no sumcheck in progress (lfplus_mlsumcheck_begin)");
    if (!r_last || !evals_out) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_final: null argument");
    if (s->done < s->nvars) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_final: " + std::to_string(s->nvars - s->done) + " rounds are still to be answered");
    if (*r_last >= P) return fail(c, LFPLUS_E_ARG, "lfplus_mlsumcheck_final: non-canonical challenge");
    HIPCHK(c, hipSetDevice(c->device));
    lfp::launch_mls_final(s->cur, s->cur_len, s->T, to_mont(*r_last), s->res, c->st);      // (cur holds two entries per table: nvars - 1 variables are fixed)
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s->hres, s->res, (size_t)s->T * 16 * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    memcpy(evals_out, s->hres, (size_t)s->T * 16 * 8);
    return LFPLUS_OK;
}
// prove_as_subprotocol: absorb(nvars), absorb(degree), per round absorb_slice(evaluations), get_challenge, absorb(challenge) -- the loop over the split form
int prove_impl(lfplus_ctx *c, lfplus_transcript *tr, const lfplus_vpoly *vp, const uint64_t *tables, uint64_t *msgs, uint64_t *point, uint64_t *fin, Origin o, const char *who) {
    if (!tr || !msgs || !point) return fail(c, LFPLUS_E_ARG, std::string(who) + ": null argument");
    int rc = begin_impl(c, vp, tables, o, true, who);      // (every refusal happens in here: the transcript is untouched then)
    if (rc) return rc;
    const u32 nv = vp->nvars, np = vp->degree + 1;
    u64 e[16] = {0};
    e[0] = nv; lfplus_transcript_absorb(tr, e, 1);
    e[0] = vp->degree; lfplus_transcript_absorb(tr, e, 1);
    u64 r = 0;
    for (u32 i = 0; i < nv && !rc; i++) {
        u64 *m = msgs + (size_t)i * np * 16;
        rc = round_impl(c, i ? &r : nullptr, m);
        if (rc) break;
        lfplus_transcript_absorb(tr, m, np);
        lfplus_transcript_challenge(tr, &r);
        e[0] = r; lfplus_transcript_absorb(tr, e, 1);
        point[i] = r;
    }
    if (!rc && fin) rc = final_impl(c, &r, fin);
    const std::string keep = c->err;
    lfp_mls_drop(c);
    if (rc) c->err = keep;
    return rc;
}
int no_ctx() {      // a NULL context: without a device none can exist (lfplus_ctx_create said so), and that is the answer
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 1) { (void)hipGetLastError(); return LFPLUS_E_NO_DEVICE; }
    return LFPLUS_E_ARG;
}
int oom(lfplus_ctx *c, const char *m) {
    try { c->err = m; } catch (...) {}
    return LFPLUS_E_HIP;
}
}  // namespace

void lfp_mls_drop(lfplus_ctx *c) {
    if (!c || !c->mls) return;
    mls_free(c, c->mls);
    c->mls = nullptr;
}

extern "C" int lfplus_mlsumcheck_begin(lfplus_ctx *c, const lfplus_vpoly *vp, const uint64_t *tables) {
    if (!c) return no_ctx();
    LFP_GUARD(begin_impl(c, vp, tables, Origin::host, false, "lfplus_mlsumcheck_begin"), oom(c, "lfplus_mlsumcheck_begin: out of host memory"))
}
extern "C" int lfplus_mlsumcheck_begin_device(lfplus_ctx *c, const lfplus_vpoly *vp, const uint64_t *tables) {
    if (!c) return no_ctx();
    LFP_GUARD(begin_impl(c, vp, tables, Origin::device, false, "lfplus_mlsumcheck_begin_device"), oom(c, "lfplus_mlsumcheck_begin_device: out of host memory"))
}
extern "C" int lfplus_mlsumcheck_round(lfplus_ctx *c, const uint64_t *r_prev, uint64_t *evals_out) {
    if (!c) return no_ctx();
    LFP_GUARD(round_impl(c, r_prev, evals_out), oom(c, "lfplus_mlsumcheck_round: out of host memory"))
}
extern "C" int lfplus_mlsumcheck_final(lfplus_ctx *c, const uint64_t *r_last, uint64_t *evals_out) {
    if (!c) return no_ctx();
    LFP_GUARD(final_impl(c, r_last, evals_out), oom(c, "lfplus_mlsumcheck_final: out of host memory"))
}
extern "C" int lfplus_mlsumcheck_end(lfplus_ctx *c) {
    if (!c) return LFPLUS_E_ARG;
    lfp_mls_drop(c);
    return LFPLUS_OK;
}
extern "C" int lfplus_mlsumcheck_prove(lfplus_ctx *c, lfplus_transcript *tr, const lfplus_vpoly *vp, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out,
                                       uint64_t *final_out) {
    if (!c) return no_ctx();
    LFP_GUARD(prove_impl(c, tr, vp, tables, msgs_out, point_out, final_out, Origin::host, "lfplus_mlsumcheck_prove"), oom(c, "lfplus_mlsumcheck_prove: out of host memory"))
}
extern "C" int lfplus_mlsumcheck_prove_device(lfplus_ctx *c, lfplus_transcript *tr, const lfplus_vpoly *vp, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out,
                                           uint64_t *final_out) {
    if (!c) return no_ctx();
    LFP_GUARD(prove_impl(c, tr, vp, tables, msgs_out, point_out, final_out, Origin::device, "lfplus_mlsumcheck_prove_device"), oom(c, "lfplus_mlsumcheck_prove_device: out of host memory"))
}
