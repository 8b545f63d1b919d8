// lf_prover.cpp -- the chained NIFS prover as an object of the C ABI (include/lfhip_prover.h): host code over the entry points of lfhip.h, which are the
// ring-generic bodies of lf_ring_host.h behind their argument and external-basis handling.  The object adds the chain state of nifs/tests.rs:58-117 (the
// accumulator LCCCS on the host, its folded witness and the fresh witness as device handles, the pending ingest job) and the rules a hand-rolled loop gets
// wrong: one pending instance, no job left behind at destroy, no step on a context whose constraint system or matrix was loaded again.
// The fresh witness is committed at the head of the prove on the context's main lane (lf_witness_commit), under either value of `flags`: committing inside
// the ingest job on lane 2 was built, measured slower and removed.
#include <exception>
#include <string>
#include <vector>

#include "lf_ctx.h"

namespace {
bool same_params(const lf_params &a, const lf_params &b) {
    return a.s == b.s && a.wit_len == b.wit_len && a.l == b.l && a.L == b.L && a.K == b.K && a.b == b.b && a.B == b.B && a.kappa == b.kappa && a.t == b.t &&
           a.q == b.q && a.d == b.d;
}
}  // namespace

struct lf_prover {
    lf_ctx *c = nullptr;
    unsigned flags = 0;               // recorded; both values commit at the head of the prove
    // the context as it was at create
    lf_params P{};
    size_t N = 0;
    uint32_t kappa = 0;
    uint64_t gen = 0;
    int ring = 0;
    size_t RE = 0, lc_words = 0, cm_words = 0, x_words = 0;
    // chain state
    bool ready = false, failed = false;
    std::vector<uint64_t> acc;        // the accumulator's LCCCS (caller's basis)
    lf_witness *w_acc = nullptr;
    bool pending = false;
    lf_witness_job *job = nullptr;    // the ingest still running (host ingests), joined by check_fresh or prove
    lf_witness *w_new = nullptr;
    bool have_cm = false;
    std::vector<uint64_t> cccs;       // cm || x_ccs of the pending instance; cm valid once have_cm
    uint64_t steps = 0;
    std::string err;

    int fail(int rc, const std::string &msg) {
        err = msg + ": " + lf_strerror(rc);
        return rc;
    }
    // the refusals every call starts with: a FAILED prover, a context that is not the one of create any more
    int enter(const char *call) {
        if (failed) return fail(LF_ERR_STATE, std::string(call) + ": the prover failed inside a step and holds no usable chain (destroy it)");
        CtxCoreBase &k = c->core_any();
        if (!k.have_ccs || !k.A_loaded || k.setup_gen != gen || !same_params(k.P, P) || k.N != N || k.kappa != kappa)
            return fail(LF_ERR_STATE, std::string(call) + ": the context's constraint system or matrix was replaced since lf_prover_create");
        return LF_OK;
    }
    // a refusal of ingest, check_fresh or prove: the pending instance goes (its w_ccs is not borrowed any more), the accumulator stays
    int refuse(int rc, const std::string &msg) {
        drop_pending();
        return fail(rc, msg);
    }
    void drop_pending() {
        if (job) (void)lf_witness_job_finish(job, nullptr);   // waits for the worker and frees what it made
        job = nullptr;
        if (w_new) lf_witness_free(w_new);
        w_new = nullptr;
        pending = have_cm = false;
    }
    // the pending witness, joined and committed: cccs = cm || x_ccs afterwards.  An error drops the pending instance
    int fresh_ready(const char *call) {
        if (job) {
            lf_witness_job *j = job;
            job = nullptr;
            const int rc = lf_witness_job_finish(j, &w_new);
            if (rc != LF_OK) { w_new = nullptr; drop_pending(); return fail(rc, std::string(call) + ": the ingest job failed (lf_witness_from_w_ccs)"); }
        }
        if (!have_cm) {
            const int rc = lf_witness_commit(c, w_new, cccs.data());
            if (rc != LF_OK) { drop_pending(); return fail(rc, std::string(call) + ": lf_witness_commit of the fresh witness"); }
            have_cm = true;
        }
        return LF_OK;
    }
    bool ring_of(const lf_transcript *t) const { return (c->bb != nullptr) == (t->bb != nullptr); }
};

// no C++ exception leaves the library
#define LF_PROVER_GUARD(pr, body)                                                              \
    try { body }                                                                               \
    catch (const std::exception &e) { return (pr)->fail(LF_ERR_HIP, std::string("exception: ") + e.what()); } \
    catch (...) { return (pr)->fail(LF_ERR_HIP, "exception"); }

extern "C" {

int lf_prover_create(lf_ctx *c, unsigned flags, lf_prover **out) {
    if (out) *out = nullptr;
    if (!c || !out || (flags & ~(unsigned)LF_PROVER_COMMIT_INLINE)) return LF_ERR_INVALID;
    try {
        CtxCoreBase &k = c->core_any();
        if (!k.have_ccs || !k.A_loaded) return LF_ERR_STATE;
        if (k.sh_world > 1) return LF_ERR_UNSUPPORTED;
        lf_prover *p = new lf_prover();
        p->c = c;
        p->flags = flags;
        p->P = k.P; p->N = k.N; p->kappa = k.kappa; p->gen = k.setup_gen;
        p->ring = lf_ctx_ring(c);
        p->RE = (size_t)lf_ring_words(p->ring);
        p->lc_words = lf_lcccs_len_ring(&p->P, p->ring) * p->RE;
        p->cm_words = (size_t)p->P.kappa * p->RE;
        p->x_words = (size_t)p->P.l * p->RE;
        p->cccs.assign(p->cm_words + p->x_words, 0);
        *out = p;
        return LF_OK;
    } catch (...) { return LF_ERR_HIP; }
}

void lf_prover_destroy(lf_prover *p) {
    if (!p) return;
    try {
        p->drop_pending();
        if (p->w_acc) lf_witness_free(p->w_acc);
    } catch (...) {}
    delete p;
}

const char *lf_prover_last_error(const lf_prover *p) { return p ? p->err.c_str() : "null prover"; }

uint64_t lf_prover_steps(const lf_prover *p) { return p ? p->steps : 0; }

int lf_prover_init(lf_prover *p, lf_transcript *t, const uint64_t *w_ccs, const uint64_t *x_ccs, uint64_t *lcccs_out, uint64_t *lin_proof_out) {
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        if (!t || !w_ccs || !x_ccs || !lcccs_out || !lin_proof_out) return p->fail(LF_ERR_INVALID, "lf_prover_init: NULL argument");
        RET(p->enter("lf_prover_init"));
        if (!p->ring_of(t)) return p->fail(LF_ERR_INVALID, "lf_prover_init: the transcript belongs to the other ring");
        if (p->ready) return p->fail(LF_ERR_STATE, "lf_prover_init: the prover has an accumulator already");
        lf_witness *w = nullptr;
        int rc = lf_witness_from_w_ccs(p->c, w_ccs, &w);
        if (rc != LF_OK) return p->fail(rc, "lf_prover_init: lf_witness_from_w_ccs");
        std::vector<uint64_t> cccs(p->cm_words + p->x_words);
        rc = lf_witness_commit(p->c, w, cccs.data());
        if (rc != LF_OK) { lf_witness_free(w); return p->fail(rc, "lf_prover_init: lf_witness_commit"); }
        memcpy(cccs.data() + p->cm_words, x_ccs, p->x_words * 8);
        std::vector<uint64_t> lc(p->lc_words);
        rc = lf_linearize(p->c, t, cccs.data(), w, lc.data(), lin_proof_out);
        if (rc != LF_OK) {   // the transcript may have been advanced: there is no chain to go on with
            lf_witness_free(w);
            p->failed = true;
            return p->fail(rc, "lf_prover_init: lf_linearize");
        }
        memcpy(lcccs_out, lc.data(), p->lc_words * 8);
        p->acc.swap(lc);
        p->w_acc = w;
        p->ready = true;
        p->steps = 0;
        p->err.clear();
        return LF_OK;
    })
}

static int prover_resume(lf_prover *p, const uint64_t *lcccs, const uint64_t *f_ntt, bool dev) {
    const char *call = dev ? "lf_prover_resume_dev" : "lf_prover_resume";
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        if (!lcccs || !f_ntt) return p->fail(LF_ERR_INVALID, std::string(call) + ": NULL argument");
        RET(p->enter(call));
        if (p->ready) return p->fail(LF_ERR_STATE, std::string(call) + ": the prover has an accumulator already");
        lf_witness *w = nullptr;
        const int rc = dev ? lf_witness_from_f_dev(p->c, f_ntt, &w) : lf_witness_from_f(p->c, f_ntt, &w);
        if (rc != LF_OK) return p->fail(rc, std::string(call) + (dev ? ": lf_witness_from_f_dev" : ": lf_witness_from_f"));
        p->acc.assign(lcccs, lcccs + p->lc_words);
        p->w_acc = w;
        p->ready = true;
        p->steps = 0;
        p->err.clear();
        return LF_OK;
    })
}
int lf_prover_resume(lf_prover *p, const uint64_t *lcccs, const uint64_t *f_ntt) { return prover_resume(p, lcccs, f_ntt, false); }
int lf_prover_resume_dev(lf_prover *p, const uint64_t *lcccs, const uint64_t *f_ntt_dev) { return prover_resume(p, lcccs, f_ntt_dev, true); }

static int prover_ingest(lf_prover *p, const uint64_t *w_ccs, const uint64_t *x_ccs, bool dev) {
    const char *call = dev ? "lf_prover_ingest_dev" : "lf_prover_ingest";
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        if (!w_ccs || !x_ccs) return p->refuse(LF_ERR_INVALID, std::string(call) + ": NULL argument");
        RET(p->enter(call));
        if (!p->ready) return p->refuse(LF_ERR_STATE, std::string(call) + ": no accumulator (lf_prover_init / lf_prover_resume first)");
        if (p->pending) return p->refuse(LF_ERR_STATE, std::string(call) + ": an instance is pending already");
        int rc;
        if (dev) rc = lf_witness_from_w_ccs_dev(p->c, w_ccs, &p->w_new);
        else rc = lf_witness_from_w_ccs_begin(p->c, w_ccs, &p->job);
        if (rc != LF_OK) {
            p->w_new = nullptr; p->job = nullptr;
            return p->fail(rc, std::string(call) + (dev ? ": lf_witness_from_w_ccs_dev" : ": lf_witness_from_w_ccs_begin"));
        }
        memcpy(p->cccs.data() + p->cm_words, x_ccs, p->x_words * 8);
        p->pending = true;
        p->have_cm = false;
        p->err.clear();
        return LF_OK;
    })
}
int lf_prover_ingest(lf_prover *p, const uint64_t *w_ccs, const uint64_t *x_ccs) { return prover_ingest(p, w_ccs, x_ccs, false); }
int lf_prover_ingest_dev(lf_prover *p, const uint64_t *w_ccs_dev, const uint64_t *x_ccs) { return prover_ingest(p, w_ccs_dev, x_ccs, true); }

int lf_prover_check_fresh(lf_prover *p, uint64_t bound, unsigned *failed, uint64_t *first_bad) {
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        if (!failed || !first_bad) return p->refuse(LF_ERR_INVALID, "lf_prover_check_fresh: NULL argument");
        RET(p->enter("lf_prover_check_fresh"));
        if (!p->ready || !p->pending) return p->refuse(LF_ERR_STATE, "lf_prover_check_fresh: no pending instance (lf_prover_ingest first)");
        RET(p->fresh_ready("lf_prover_check_fresh"));
        const int rc = lf_cccs_check(p->c, p->cccs.data(), p->w_new, bound, failed, first_bad);
        if (rc == LF_ERR_REJECT) return p->fail(rc, "lf_prover_check_fresh: the pending instance is not in R_CCCS");
        if (rc != LF_OK) { p->drop_pending(); return p->fail(rc, "lf_prover_check_fresh: lf_cccs_check"); }
        p->err.clear();
        return LF_OK;
    })
}

int lf_prover_prove(lf_prover *p, lf_transcript *t, uint64_t *cccs_out, uint64_t *lcccs_out, uint64_t *proof_out) {
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        if (!t || !lcccs_out || !proof_out) return p->refuse(LF_ERR_INVALID, "lf_prover_prove: NULL argument");
        RET(p->enter("lf_prover_prove"));
        if (!p->ring_of(t)) return p->refuse(LF_ERR_INVALID, "lf_prover_prove: the transcript belongs to the other ring");
        if (!p->ready || !p->pending) return p->refuse(LF_ERR_STATE, "lf_prover_prove: no pending instance (lf_prover_ingest first)");
        RET(p->fresh_ready("lf_prover_prove"));
        if (cccs_out) memcpy(cccs_out, p->cccs.data(), p->cccs.size() * 8);
        std::vector<uint64_t> lc(p->lc_words);
        lf_witness *w_next = nullptr;
        const int rc = lf_fold_step(p->c, t, p->acc.data(), p->w_acc, p->cccs.data(), p->w_new, lc.data(), &w_next, proof_out);
        if (rc != LF_OK) {   // the transcript may have been advanced: the chain cannot go on from here
            if (w_next) lf_witness_free(w_next);
            p->drop_pending();
            p->failed = true;
            return p->fail(rc, "lf_prover_prove: lf_fold_step");
        }
        memcpy(lcccs_out, lc.data(), p->lc_words * 8);
        lf_witness_free(p->w_acc);     // (planes back to the recycle pool: the next ingest and the next step draw from it)
        p->drop_pending();
        p->acc.swap(lc);
        p->w_acc = w_next;
        p->steps++;
        p->err.clear();
        return LF_OK;
    })
}

static int prover_accumulator(lf_prover *p, uint64_t *lcccs_out, uint64_t *f_out, bool dev) {
    const char *call = dev ? "lf_prover_accumulator_dev" : "lf_prover_accumulator";
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        RET(p->enter(call));
        if (!p->ready) return p->fail(LF_ERR_STATE, std::string(call) + ": no accumulator (lf_prover_init / lf_prover_resume first)");
        if (f_out) {
            const int rc = dev ? lf_witness_get_f_dev(p->c, p->w_acc, f_out) : lf_witness_get_f(p->c, p->w_acc, f_out);
            if (rc != LF_OK) return p->fail(rc, std::string(call) + (dev ? ": lf_witness_get_f_dev" : ": lf_witness_get_f"));
        }
        if (lcccs_out) memcpy(lcccs_out, p->acc.data(), p->lc_words * 8);
        p->err.clear();
        return LF_OK;
    })
}
int lf_prover_accumulator(lf_prover *p, uint64_t *lcccs_out, uint64_t *f_ntt_out) { return prover_accumulator(p, lcccs_out, f_ntt_out, false); }
int lf_prover_accumulator_dev(lf_prover *p, uint64_t *lcccs_out, uint64_t *f_ntt_dev_out) { return prover_accumulator(p, lcccs_out, f_ntt_dev_out, true); }

int lf_prover_decide(lf_prover *p, uint64_t bound, unsigned *failed) {
    if (!p) return LF_ERR_INVALID;
    LF_PROVER_GUARD(p, {
        if (!failed) return p->fail(LF_ERR_INVALID, "lf_prover_decide: NULL argument");
        RET(p->enter("lf_prover_decide"));
        if (!p->ready) return p->fail(LF_ERR_STATE, "lf_prover_decide: no accumulator (lf_prover_init / lf_prover_resume first)");
        const int rc = lf_lcccs_check(p->c, p->acc.data(), p->w_acc, bound, failed);
        if (rc != LF_OK) return p->fail(rc, rc == LF_ERR_REJECT ? "lf_prover_decide: the accumulator is not in R_LCCCS" : "lf_prover_decide: lf_lcccs_check");
        p->err.clear();
        return LF_OK;
    })
}

}  // extern "C"
