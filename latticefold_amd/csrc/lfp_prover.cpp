// lfp_prover.cpp -- PlusProver / PlusVerifier (crates/latticefold-plus/src/plus.rs:15-146) as objects behind the C ABI, and the flat PlusProof.
//
// Host code only, written against include/lfplus.h alone: the prover is a schedule over the context-level entry points (lfp_capi.cpp, lfp_protocol.cpp), the
// verifier a sequence of the three host verifiers.  What the schedule has to get right:
//   * contexts 0 and 1 hold the accumulator halves (F0, F1) once a prove has run, the fresh instances of the next prove go into the contexts after them;
//   * RgInstance::from_f needs no challenge: it is enqueued on every context's second stream as soon as the witness is resident and runs next to the
//     linearizations' latency-bound rounds (lfplus_mlin collects the results);
//   * host witnesses cross PCIe on a worker thread, one after the other, while this thread linearizes the instances that have arrived;
//   * a prove that fails half way has advanced the Fiat-Shamir transcript: the object refuses to continue;
//   * the _dev twins (device-origin z, f, F0 / F1) go through the contexts' own _dev entry points: the bodies below take the origin, and a device witness is
//     copied and checked at once, on this thread (a device-to-device pass is tens of microseconds: there is nothing for a worker to hide).
//   * the instances are ComR1CS (lfplus_prover_create) or committed CCS instances of one shape (lfplus_prover_create_ccs): everything that differs between the
//     two is in `Lin` below, and the layout, the verifier and the prover bodies are written over it once.
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/lfplus.h"
#include "lfp_guard.h"

// THE pointer check of a device-origin array (lfp_capi.cpp; dev_array_check behind it): LFPLUS_OK, or LFPLUS_E_ARG with the context's message set
int lfp_dev_ptr_check(lfplus_ctx *c, const void *p, uint64_t elems, const char *who);
// THE refusals of a CCS shape (lfp_protocol.cpp; lfp_ccs.h behind it): LFPLUS_OK with *deg = max |S_i|, or LFPLUS_E_ARG
int lfp_ccs_shape_check(const lfplus_ccs *shape, uint32_t *deg);

namespace {
enum class Origin { host, device };      // where the O(n) arrays of a call live (include/lfplus.h "device-resident callers")
typedef uint64_t u64;
typedef uint32_t u32;
constexpr u64 D = LFPLUS_D;

// ---- the linearization of a prover: everything that differs between ComR1CS (r1cs.rs:62-163) and a committed CCS instance (lfplus_ccs) -- the sizes of the
// per-instance fields, the header, and the three calls (linearize, verify, check).  Layout, verify_impl and the prover bodies below are written over it once.
struct Lin {
    u32 nM = 3;          // matrices of the fold's tail (mlin, decompose); a CCS shape's t
    u32 np = 4;          // evaluations per sumcheck round: d + 2 (R1CS: degree 3)
    u32 nev = 4;         // ring elements of `evals`: v and one per matrix of the linearization (R1CS: always A, B, C)
    bool ccs = false;
    std::vector<u32> S_off, S_idx;      // the prover's copy of the shape
    std::vector<u64> c;
    static Lin r1cs(u32 nM) { Lin l; l.nM = nM; return l; }
    // the refusals of lfplus_ccs_linearize's shape, in its order (lfp_ccs.h)
    static bool from_ccs(const lfplus_ccs *s, Lin &l) {
        u32 deg = 0;
        if (lfp_ccs_shape_check(s, &deg) != LFPLUS_OK) return false;
        l.nM = s->t; l.np = deg + 2; l.nev = 1 + s->t; l.ccs = true;
        l.S_off.assign(s->S_off, s->S_off + s->q + 1);
        l.S_idx.assign(s->S_idx, s->S_idx + s->S_off[s->q]);
        l.c.assign(s->c, s->c + (size_t)s->q * D);
        return true;
    }
    lfplus_ccs shape() const { return lfplus_ccs{nM, (u32)(S_off.size() - 1), S_off.data(), S_idx.data(), c.data()}; }
    u32 header_words() const { return ccs ? LFPLUS_PROOF_HEADER_CCS : LFPLUS_PROOF_HEADER; }
    void header(u64 *h, const lfplus_params *p, u32 nvars, u32 L, u32 nfresh) const {
        const u64 common[8] = {ccs ? LFPLUS_PROOF_MAGIC_CCS : LFPLUS_PROOF_MAGIC, L, nfresh, nvars, p->k, p->l, p->kappa, nM};
        memcpy(h, common, sizeof common);
        if (ccs) { h[8] = S_off.size() - 1; h[9] = np - 2; h[10] = S_off.back(); h[11] = 0; }
    }
    int linearize(lfplus_ctx *ctx, lfplus_transcript *tr, u64 *msgs, u64 *ro, u64 *evals) const {      // on the resident witness and matrices
        if (!ccs) return lfplus_r1cs_linearize(ctx, tr, nullptr, nullptr, nullptr, msgs, ro, evals);
        const lfplus_ccs s = shape();
        return lfplus_ccs_linearize(ctx, tr, &s, nullptr, nullptr, nullptr, msgs, ro, evals);
    }
    int verify(lfplus_transcript *tr, u32 nvars, const u64 *msgs, const u64 *evals, u64 *ro, int *st) const {
        if (!ccs) return lfplus_r1cs_verify(tr, nvars, msgs, evals, ro, st);
        const lfplus_ccs s = shape();
        return lfplus_ccs_verify(tr, nvars, &s, msgs, evals, ro, st);
    }
    int check(lfplus_ctx *ctx, const u64 *cm_f, u64 bound, unsigned *failed, u64 *first_bad, u64 *absmax) const {
        if (!ccs) return lfplus_r1cs_check(ctx, cm_f, nullptr, nullptr, nullptr, bound, failed, first_bad, absmax);
        const lfplus_ccs s = shape();
        return lfplus_ccs_check(ctx, cm_f, &s, nullptr, nullptr, nullptr, bound, failed, first_bad, absmax);
    }
};

// ---- the flat proof ------------------------------------------------------------------------------------------------------------------------------------
bool shape_ok(const lfplus_params *p, u64 n, u32 nM, u32 L, u32 nfresh, u32 *nvars_out) {
    if (!p || n < 2 || n > (1ull << 32) || (n & (n - 1))) return false;
    if (!L || L > 4096 || nfresh > L || !p->k || p->k > 16 || !p->l || p->l > 64 || !p->kappa || p->kappa > 64 || nM > 64) return false;
    u32 nvars = 0;
    while ((1ull << nvars) < n) nvars++;
    *nvars_out = nvars;
    return true;
}
// field indices after the 3 nfresh linearization-proof fields
enum { CM_R, CM_MSGS, CM_E, CM_B, CM_V, CM_A, CM_BB, CM_C, CM_COMH, CM_PA, CM_PB, CM_EA, CM_EB, CM_CMG, CM_RO, CM_VO, CM_FCOMS, X_CMG, X_RO, X_VO, D_C0, D_C1, D_V0, D_V1, NTAIL };
struct Layout {
    u32 nvars = 0;
    std::vector<u64> off, len;
    u64 total = 0;
    bool build(const lfplus_params *p, u64 n, const Lin &lin, u32 L, u32 nfresh) {
        const u32 nM = lin.nM;
        if (!shape_ok(p, n, nM, L, nfresh, &nvars)) return false;
        const u64 nv = nvars, kap = p->kappa, q = 1 + (u64)nM, per = 4 + 4 * (u64)nM, l = L;
        len.clear();
        for (u32 i = 0; i < nfresh; i++) { len.push_back(nv * lin.np * D); len.push_back(nv); len.push_back(lin.nev * D); }
        const u64 tail[NTAIL] = {nv, nv * 4 * D, q * l * p->k * D * D, l * D, l * D, l * q, l * q * D, l * q * D, l * kap * D, nv * 3 * D, nv * 3 * D, l * per * D, l * per * D,
                                 l * kap * D, 2 * nv, l * q * 2 * D, l * 3 * kap * D, kap * D, 2 * nv, q * 2 * D, kap * D, kap * D, q * 2 * D, q * 2 * D};
        len.insert(len.end(), tail, tail + NTAIL);
        off.resize(len.size());
        total = lin.header_words();
        for (size_t i = 0; i < len.size(); i++) { off[i] = total; total += len[i]; }      // (every factor is bounded by the envelope: < 2^40 words)
        return true;
    }
};
bool header_ok(const u64 *proof, const lfplus_params *p, const Lin &lin, u32 nvars, u32 L, u32 nfresh) {
    u64 h[LFPLUS_PROOF_HEADER_CCS];
    lin.header(h, p, nvars, L, nfresh);
    return memcmp(proof, h, (size_t)lin.header_words() * 8) == 0;
}
}  // namespace

extern "C" uint32_t lfplus_proof_fields(uint32_t nfresh) { return 3 * nfresh + NTAIL; }
static uint64_t proof_len_impl(const lfplus_params *p, uint64_t n, const Lin &lin, uint32_t L, uint32_t nfresh) {
    Layout lay;
    return lay.build(p, n, lin, L, nfresh) ? lay.total : 0;
}
static int proof_layout_impl(const lfplus_params *p, uint64_t n, const Lin &lin, uint32_t L, uint32_t nfresh, uint64_t *offsets, uint64_t *lengths, uint32_t nfields) {
    Layout lay;
    if (!offsets || !lengths || !lay.build(p, n, lin, L, nfresh) || nfields != lay.len.size()) return LFPLUS_E_ARG;
    memcpy(offsets, lay.off.data(), lay.off.size() * 8);
    memcpy(lengths, lay.len.data(), lay.len.size() * 8);
    return LFPLUS_OK;
}

// ---- PlusVerifier::verify ------------------------------------------------------------------------------------------------------------------------------
static int verify_impl(const lfplus_params *p, uint64_t n, const Lin &lin, uint32_t L, uint32_t nfresh, lfplus_transcript *tr, const uint64_t *proof,
                             uint64_t proof_words, int *which, int *stage) {
    if (which) *which = -1;
    if (stage) *stage = 0;
    Layout lay;
    const u32 nM = lin.nM;
    if (!tr || !proof || !lay.build(p, n, lin, L, nfresh)) return LFPLUS_E_ARG;
    if (proof_words != lay.total || !header_ok(proof, p, lin, lay.nvars, L, nfresh)) return LFPLUS_E_ARG;      // (nothing below the header has been read)
    const u32 nvars = lay.nvars;
    int st = 0;
    std::vector<u64> ro(2 * (size_t)nvars);
    for (u32 i = 0; i < nfresh; i++) {
        const int rc = lin.verify(tr, nvars, proof + lay.off[3 * i], proof + lay.off[3 * i + 2], ro.data(), &st);
        if (rc) { if (which) *which = (int)i; if (stage) *stage = st; return rc; }
    }
    const size_t t0 = 3 * (size_t)nfresh;
    auto fld = [&](int i) { return proof + lay.off[t0 + (size_t)i]; };
    std::vector<const u64 *> fcoms(L);
    for (u32 i = 0; i < L; i++) fcoms[i] = fld(CM_FCOMS) + (size_t)i * 3 * p->kappa * D;
    std::vector<u64> cm_g(lay.len[t0 + CM_CMG]), vo(lay.len[t0 + CM_VO]);      // the folded instance as the verifier recomputes it (CmProof::verify's return value)
    int rc = lfplus_cm_verify(tr, nvars, L, p->k, p->l, p->kappa, nM, fcoms.data(), fld(CM_MSGS), fld(CM_E), fld(CM_B), fld(CM_V), fld(CM_A), fld(CM_BB), fld(CM_C), fld(CM_COMH),
                              fld(CM_PA), fld(CM_PB), fld(CM_EA), fld(CM_EB), cm_g.data(), ro.data(), vo.data(), &st);
    if (rc) { if (which) *which = (int)nfresh; if (stage) *stage = st; return rc; }
    rc = lfplus_decomp_verify(fld(D_C0), fld(D_C1), p->kappa, fld(D_V0), fld(D_V1), 1 + nM, fld(X_CMG), fld(X_VO), p->B, &st);
    if (rc) { if (which) *which = (int)nfresh + 1; if (stage) *stage = st; return rc; }
    return LFPLUS_OK;
}

// ---- PlusProver ----------------------------------------------------------------------------------------------------------------------------------------
struct lfplus_prover {
    int device = 0;
    lfplus_params p{};
    u64 n = 0;
    Lin lin;                              // the linearization of its instances: ComR1CS (lfplus_prover_create) or a CCS shape (lfplus_prover_create_ccs)
    std::vector<lfplus_ctx *> ctxs;
    lfplus_transcript *tr = nullptr;      // borrowed
    u32 nacc = 0;                         // 0 before the first prove, 2 after it: contexts [0, nacc) hold the accumulator
    u32 nfresh = 0;                       // instances named by ingest / set_instances for the next prove, in contexts [nacc, nacc + nfresh)
    u32 last_L = 0, last_nfresh = 0;      // shape of the last proof (lfplus_prover_decide)
    bool failed = false;
    std::string err, why;                 // why: the error that made the prover fail
    std::vector<std::vector<u64>> cm_f;   // set_instances: the callers' commitments (empty: not given)
    // the upload worker (set_instances): arrived = instances resident so far, up_rc != 0: the upload of instance `arrived` failed
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    u32 arrived = 0;
    int up_rc = 0;
    std::string up_err;
    void join() { if (worker.joinable()) worker.join(); }
};

static int pfail(lfplus_prover *pr, int rc, const std::string &m) {
    pr->err = m;
    return rc;
}
static int pdead(lfplus_prover *pr, const char *who) {
    return pfail(pr, LFPLUS_E_ARG, std::string(who) + ": this prover failed earlier (" + pr->why + ") -- its transcript and contexts are half-advanced, build a new prover");
}
// an error inside ingest / set_instances / prove: the object survives (the reference panics), so it must refuse to continue from this state
static int pbreak(lfplus_prover *pr, int rc, const std::string &m) {
    pr->join();
    pr->failed = true;
    pr->why = m;
    return pfail(pr, rc, m);
}
// the same when memory itself ran out: the message is a literal, nothing is formatted
static int pbreak_nothrow(lfplus_prover *pr, const char *m) {
    try { pr->join(); } catch (...) {}
    pr->failed = true;
    try { pr->why = m; pr->err = m; } catch (...) {}
    return LFPLUS_E_HIP;
}
static std::string ctx_err(lfplus_ctx *c, const char *who) { return std::string(who) + ": " + lfplus_last_error(c); }

// both creators: `lin` is the linearization the caller's arguments name (its refusals are the caller's, before this body)
static int prover_create_impl(int device, const lfplus_params *params, const uint64_t *A, uint64_t seed, uint64_t n, const Lin &lin, const uint32_t *const *rowptr,
                                    const uint32_t *const *col, const uint64_t *const *val, uint32_t ncomp, lfplus_transcript *transcript, lfplus_prover **out) {
    const u32 nM = lin.nM;
    u32 nvars = 0;
    if (!transcript || !shape_ok(params, n, nM, 1, 0, &nvars) || !rowptr || !col || !val || ncomp > 4094) return LFPLUS_E_ARG;
    if (params->b < 2 || params->B < 2) return LFPLUS_E_ARG;
    lfplus_prover *pr = new lfplus_prover;
    struct Guard { lfplus_prover *p; ~Guard() { if (p) lfplus_prover_destroy(p); } } guard{pr};      // (an early return or a throw below releases what exists so far)
    pr->device = device; pr->p = *params; pr->n = n; pr->lin = lin; pr->tr = transcript;
    int rc = LFPLUS_OK;
    for (u32 i = 0; i < 2 + ncomp && !rc; i++) {
        lfplus_ctx *c = nullptr;
        if ((rc = lfplus_ctx_create(device, &c))) break;
        pr->ctxs.push_back(c);
        if (i == 0) {
            rc = A ? lfplus_set_matrix(c, A, params->kappa, n) : lfplus_matrix_generate(c, seed, params->kappa, n);
            if (!rc) rc = lfplus_set_matrices(c, n, nM, rowptr, col, val);
        } else {
            rc = lfplus_share_matrix(c, pr->ctxs[0]);
            if (!rc) rc = lfplus_share_matrices(c, pr->ctxs[0]);
        }
    }
    if (rc) return rc;
    guard.p = nullptr;
    *out = pr;
    return LFPLUS_OK;
}
extern "C" void lfplus_prover_destroy(lfplus_prover *pr) {
    if (!pr) return;
    pr->join();      // (never leave the worker writing into contexts that are about to go)
    for (size_t i = pr->ctxs.size(); i-- > 0;) lfplus_ctx_destroy(pr->ctxs[i]);
    delete pr;
}
extern "C" const char *lfplus_prover_last_error(const lfplus_prover *pr) { return pr ? pr->err.c_str() : "null prover"; }

// the checks ingest and set_instances share; 0: go on
static int fresh_ok(lfplus_prover *pr, const void *ptrs, u32 count, const char *who) {
    if (pr->failed) return pdead(pr, who);
    if (!ptrs || !count) return pfail(pr, LFPLUS_E_ARG, std::string(who) + ": no instances");
    if (pr->nfresh) return pfail(pr, LFPLUS_E_ARG, std::string(who) + ": the next prove has its instances already");
    if ((size_t)pr->nacc + count > pr->ctxs.size()) return pfail(pr, LFPLUS_E_ARG, std::string(who) + ": more instances than contexts (ncomp)");
    return LFPLUS_OK;
}
// every device-origin array of a call against THE pointer check, before any context is touched: a refusal is a shape error, the prover stays usable
static int dev_arrays_ok(lfplus_prover *pr, Origin o, const uint64_t *const *ptrs, u32 count, u64 elems, const char *who) {
    for (u32 i = 0; i < count && o == Origin::device; i++)
        if (ptrs[i] && lfp_dev_ptr_check(pr->ctxs[0], ptrs[i], elems, who)) return pfail(pr, LFPLUS_E_ARG, lfplus_last_error(pr->ctxs[0]));
    return LFPLUS_OK;
}
static int prover_ingest_impl(lfplus_prover *pr, const uint64_t *const *z, uint32_t count, uint64_t m, uint32_t l_in, uint64_t *cm_f_out, Origin o) {
    if (!pr) return LFPLUS_E_ARG;
    (void)l_in;
    int rc = fresh_ok(pr, z, count, "lfplus_prover_ingest");
    if (rc) return rc;
    for (u32 i = 0; i < count; i++)
        if (!z[i]) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_ingest: null z");
    if (!m || m > pr->n || m * pr->p.k != pr->n) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_ingest: m * k differs from n");      // (a shape error: nothing is touched)
    if ((rc = dev_arrays_ok(pr, o, z, count, m, "lfplus_prover_ingest_dev"))) return rc;
    for (u32 i = 0; i < count; i++) {
        lfplus_ctx *c = pr->ctxs[pr->nacc + i];
        u64 *cm = cm_f_out ? cm_f_out + (size_t)i * pr->p.kappa * D : nullptr;
        rc = o == Origin::device ? lfplus_witness_from_z_dev(c, z[i], m, pr->p.B, pr->p.k, cm) : lfplus_witness_from_z(c, z[i], m, pr->p.B, pr->p.k, cm);
        if (rc) return pbreak(pr, rc, ctx_err(c, "lfplus_prover_ingest"));      // (a context may be left without its witness)
    }
    pr->cm_f.clear();
    pr->nfresh = count;
    { std::lock_guard<std::mutex> g(pr->mu); pr->arrived = count; pr->up_rc = 0; }
    return LFPLUS_OK;
}
static int prover_set_instances_impl(lfplus_prover *pr, const uint64_t *const *f, const uint64_t *const *cm_f, uint32_t count, Origin o) {
    if (!pr) return LFPLUS_E_ARG;
    int rc = fresh_ok(pr, f, count, "lfplus_prover_set_instances");
    if (rc) return rc;
    for (u32 i = 0; i < count; i++)
        if (!f[i]) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_set_instances: null f");
    if ((rc = dev_arrays_ok(pr, o, f, count, pr->n, "lfplus_prover_set_instances_dev"))) return rc;
    pr->join();
    pr->cm_f.assign(count, std::vector<u64>());
    for (u32 i = 0; i < count && cm_f; i++)
        if (cm_f[i]) pr->cm_f[i].assign(cm_f[i], cm_f[i] + (size_t)pr->p.kappa * D);
    pr->nfresh = count;
    { std::lock_guard<std::mutex> g(pr->mu); pr->arrived = 0; pr->up_rc = 0; pr->up_err.clear(); }
    if (o == Origin::device) {      // no worker: copied and checked here, f[i] is free again on return and the prove finds every instance arrived
        for (u32 i = 0; i < count; i++) {
            lfplus_ctx *c = pr->ctxs[pr->nacc + i];
            if ((rc = lfplus_set_witness_dev(c, f[i], pr->n))) return pbreak(pr, rc, ctx_err(c, "lfplus_prover_set_instances_dev"));
        }
        std::lock_guard<std::mutex> g(pr->mu);
        pr->arrived = count;
        return LFPLUS_OK;
    }
    // the uploads, one after the other (an upload is 2.4 ms per 2^20-row witness, a linearization 2.3 ms: only the first is exposed)
    std::vector<const u64 *> src(f, f + count);
    try {
        pr->worker = std::thread([pr, src]() {
            for (size_t i = 0; i < src.size(); i++) {
                lfplus_ctx *c = pr->ctxs[pr->nacc + i];
                const int r = lfplus_set_witness(c, src[i], pr->n);
                std::lock_guard<std::mutex> g(pr->mu);
                if (r) {
                    pr->up_rc = r;
                    try { pr->up_err = lfplus_last_error(c); } catch (...) {}      // (nothing may leave the thread's function)
                    pr->cv.notify_all();
                    return;
                }
                pr->arrived = (u32)i + 1;
                pr->cv.notify_all();
            }
        });
    } catch (...) {
        return pbreak(pr, LFPLUS_E_HIP, "lfplus_prover_set_instances: no upload thread");
    }
    return LFPLUS_OK;
}
// waits until fresh instance i is resident; != 0: its upload (or an earlier one) failed
static int wait_arrived(lfplus_prover *pr, u32 i) {
    std::unique_lock<std::mutex> g(pr->mu);
    pr->cv.wait(g, [&] { return pr->arrived > i || pr->up_rc; });
    return pr->arrived > i ? 0 : pr->up_rc;
}
static int prover_prove_impl(lfplus_prover *pr, uint64_t *proof, uint64_t proof_words) {
    if (!pr) return LFPLUS_E_ARG;
    if (pr->failed) return pdead(pr, "lfplus_prover_prove");
    const u32 nacc = pr->nacc, nfresh = pr->nfresh, L = nacc + nfresh;
    Layout lay;
    if (!L) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_prove: nothing to fold (call lfplus_prover_ingest or lfplus_prover_set_instances first)");
    if (!proof || !lay.build(&pr->p, pr->n, pr->lin, L, nfresh) || proof_words != lay.total)
        return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_prove: proof_words differs from lfplus_proof_len for this prove");
    const lfplus_params &p = pr->p;
    const u32 nvars = lay.nvars;
    int rc;
    for (u32 i = 0; i < nacc; i++)
        if ((rc = lfplus_rg_from_f_async(pr->ctxs[i], p.b, p.k, p.l))) return pbreak(pr, rc, ctx_err(pr->ctxs[i], "lfplus_prover_prove (from_f)"));
    for (u32 i = 0; i < nfresh; i++) {
        lfplus_ctx *c = pr->ctxs[nacc + i];
        if ((rc = wait_arrived(pr, i))) return pbreak(pr, rc, "lfplus_prover_prove (upload): " + pr->up_err);
        if ((rc = lfplus_rg_from_f_async(c, p.b, p.k, p.l))) return pbreak(pr, rc, ctx_err(c, "lfplus_prover_prove (from_f)"));
        rc = pr->lin.linearize(c, pr->tr, proof + lay.off[3 * i], proof + lay.off[3 * i + 1], proof + lay.off[3 * i + 2]);
        if (rc) return pbreak(pr, rc, ctx_err(c, "lfplus_prover_prove (linearize)"));
    }
    pr->join();
    const size_t t0 = 3 * (size_t)nfresh;
    auto fld = [&](int i) { return proof + lay.off[t0 + (size_t)i]; };
    rc = lfplus_mlin(pr->ctxs.data(), L, pr->tr, p.b, p.k, p.l, pr->lin.nM, nullptr, nullptr, nullptr, fld(CM_R), fld(CM_MSGS), fld(CM_E), fld(CM_B), fld(CM_V), fld(CM_A),
                     fld(CM_BB), fld(CM_C), fld(CM_COMH), fld(CM_PA), fld(CM_PB), fld(CM_EA), fld(CM_EB), fld(CM_CMG), fld(CM_RO), fld(CM_VO), fld(CM_FCOMS), fld(X_CMG),
                     fld(X_VO));
    if (rc) return pbreak(pr, rc, ctx_err(pr->ctxs[0], "lfplus_prover_prove (mlin)"));
    memcpy(fld(X_RO), fld(CM_RO), 2 * (size_t)nvars * 8);
    for (u32 i = 0; i < nfresh && i < pr->cm_f.size(); i++)      // the statement's commitments against the ones the fold used
        if (!pr->cm_f[i].empty() && memcmp(pr->cm_f[i].data(), fld(CM_FCOMS) + (size_t)(nacc + i) * 3 * p.kappa * D, (size_t)p.kappa * D * 8))
            return pbreak(pr, LFPLUS_E_ARG, "lfplus_prover_prove: cm_f of a fresh instance is not the commitment of its witness");
    // ComX.ro: the two sumcheck points as pairs of ring constants (Decomp::r)
    std::vector<u64> r_a((size_t)nvars * D, 0), r_b((size_t)nvars * D, 0);
    for (u32 j = 0; j < nvars; j++) { r_a[(size_t)j * D] = fld(X_RO)[j]; r_b[(size_t)j * D] = fld(X_RO)[nvars + j]; }
    rc = lfplus_decompose_resident(pr->ctxs[0], p.B, r_a.data(), r_b.data(), pr->lin.nM, nullptr, nullptr, nullptr, pr->ctxs[0], pr->ctxs[1], fld(D_C0), fld(D_C1), fld(D_V0),
                                   fld(D_V1));
    if (rc) return pbreak(pr, rc, ctx_err(pr->ctxs[0], "lfplus_prover_prove (decompose)"));
    pr->lin.header(proof, &p, nvars, L, nfresh);
    pr->nacc = 2;
    pr->nfresh = 0;
    pr->cm_f.clear();
    pr->last_L = L; pr->last_nfresh = nfresh;
    return LFPLUS_OK;
}
static int prover_accumulator_impl(lfplus_prover *pr, uint64_t *F0, uint64_t *F1, Origin o) {
    if (!pr) return LFPLUS_E_ARG;
    if (pr->failed) return pdead(pr, "lfplus_prover_accumulator");
    if (pr->nacc != 2) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_accumulator: no accumulator (call it after a successful prove)");
    if (o == Origin::device) {
        const u64 *const both[2] = {F0, F1};
        const int rc = dev_arrays_ok(pr, o, both, 2, pr->n, "lfplus_prover_accumulator_dev");
        if (rc) return rc;
        const uintptr_t a = (uintptr_t)F0, b = (uintptr_t)F1, bytes = (uintptr_t)pr->n * D * 8;
        if (F0 && F1 && a < b + bytes && b < a + bytes) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_accumulator_dev: F0 and F1 overlap");
    }
    for (int i = 0; i < 2; i++) {
        u64 *dst = i ? F1 : F0;
        if (!dst) continue;
        const int rc = o == Origin::device ? lfplus_get_witness_dev(pr->ctxs[i], dst, pr->n) : lfplus_get_witness(pr->ctxs[i], dst, pr->n);
        if (rc) return pfail(pr, rc, ctx_err(pr->ctxs[i], "lfplus_prover_accumulator"));
    }
    return LFPLUS_OK;
}
// every context's streams wait for what `hip_stream` holds now (lfplus_ctx_wait_stream); a worker still uploading into them is joined first: one thread per context
static int prover_wait_stream_impl(lfplus_prover *pr, void *hip_stream) {
    if (pr->failed) return pdead(pr, "lfplus_prover_wait_stream");
    pr->join();
    for (lfplus_ctx *c : pr->ctxs) {
        const int rc = lfplus_ctx_wait_stream(c, hip_stream);
        if (rc) return pfail(pr, rc, ctx_err(c, "lfplus_prover_wait_stream"));
    }
    return LFPLUS_OK;
}
// Is every instance named by the last ingest / set_instances in its relation?  The relation check of this prover's linearization, where the instance lives.
// Read-only on success and on a rejection; a failed upload fails the prover as it would in the prove.
static int prover_check_fresh_impl(lfplus_prover *pr, uint64_t bound, int *ok, unsigned *failed, uint64_t *first_bad, uint64_t *absmax) {
    if (pr->failed) return pdead(pr, "lfplus_prover_check_fresh");
    if (!pr->nfresh) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_check_fresh: no fresh instances (call it between lfplus_prover_ingest / lfplus_prover_set_instances and the prove)");
    if (!ok || !failed || !first_bad || !absmax) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_check_fresh: null argument");
    int out = LFPLUS_OK;
    for (u32 i = 0; i < pr->nfresh; i++) {
        lfplus_ctx *c = pr->ctxs[pr->nacc + i];
        int rc = wait_arrived(pr, i);
        if (rc) return pbreak(pr, rc, "lfplus_prover_check_fresh (upload): " + pr->up_err);
        const u64 *cm = i < pr->cm_f.size() && !pr->cm_f[i].empty() ? pr->cm_f[i].data() : nullptr;
        failed[i] = 0; first_bad[i] = pr->n; absmax[i] = 0;
        rc = pr->lin.check(c, cm, bound, &failed[i], &first_bad[i], &absmax[i]);
        if (rc && rc != LFPLUS_E_REJECT) return pfail(pr, rc, ctx_err(c, "lfplus_prover_check_fresh"));
        ok[i] = rc == LFPLUS_OK;
        if (rc) out = LFPLUS_E_REJECT;
    }
    return out;
}
static int prover_decide_impl(lfplus_prover *pr, const uint64_t *proof, uint64_t proof_words, uint64_t bound, int *ok, unsigned *failed, uint64_t *absmax) {
    if (!pr) return LFPLUS_E_ARG;
    if (pr->failed) return pdead(pr, "lfplus_prover_decide");
    if (pr->nacc != 2 || pr->nfresh) return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_decide: no accumulator (call it after a successful prove, before the next instances)");
    Layout lay;
    if (!proof || !ok || !failed || !absmax || !lay.build(&pr->p, pr->n, pr->lin, pr->last_L, pr->last_nfresh) || proof_words != lay.total ||
        !header_ok(proof, &pr->p, pr->lin, lay.nvars, pr->last_L, pr->last_nfresh))
        return pfail(pr, LFPLUS_E_ARG, "lfplus_prover_decide: not the flat proof of this prover's last prove");
    const size_t t0 = 3 * (size_t)pr->last_nfresh;
    auto fld = [&](int i) { return proof + lay.off[t0 + (size_t)i]; };
    const u32 nvars = lay.nvars;
    std::vector<u64> r_a((size_t)nvars * D, 0), r_b((size_t)nvars * D, 0);
    for (u32 j = 0; j < nvars; j++) { r_a[(size_t)j * D] = fld(X_RO)[j]; r_b[(size_t)j * D] = fld(X_RO)[nvars + j]; }
    int out = LFPLUS_OK;
    for (int i = 0; i < 2; i++) {
        failed[i] = 0; absmax[i] = 0;
        const int rc = lfplus_linb_check(pr->ctxs[i], fld(i ? D_C1 : D_C0), r_a.data(), r_b.data(), pr->lin.nM, nullptr, nullptr, nullptr, fld(i ? D_V1 : D_V0), bound, &failed[i],
                                         &absmax[i]);
        if (rc && rc != LFPLUS_E_REJECT) return pfail(pr, rc, ctx_err(pr->ctxs[i], "lfplus_prover_decide"));
        ok[i] = rc == LFPLUS_OK;
        if (rc) out = LFPLUS_E_REJECT;
    }
    return out;
}

// ---- the entry points: the bodies above behind the exception guard ------------------------------------------------------------------------------------
extern "C" uint64_t lfplus_proof_len(const lfplus_params *p, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh) {
    LFP_GUARD(proof_len_impl(p, n, Lin::r1cs(nM), L, nfresh), 0)
}
extern "C" int lfplus_proof_layout(const lfplus_params *p, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh, uint64_t *offsets, uint64_t *lengths, uint32_t nfields) {
    LFP_GUARD(proof_layout_impl(p, n, Lin::r1cs(nM), L, nfresh, offsets, lengths, nfields), LFPLUS_E_HIP)
}
extern "C" int lfplus_verify(const lfplus_params *p, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh, lfplus_transcript *tr, const uint64_t *proof, uint64_t proof_words, int *which, int *stage) {
    LFP_GUARD(verify_impl(p, n, Lin::r1cs(nM), L, nfresh, tr, proof, proof_words, which, stage), LFPLUS_E_HIP)
}
extern "C" int lfplus_prover_create(int device, const lfplus_params *params, const uint64_t *A, uint64_t seed, uint64_t n, uint32_t nM, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val, uint32_t ncomp, lfplus_transcript *transcript, lfplus_prover **out) {
    if (!out) return LFPLUS_E_ARG;
    *out = nullptr;
    if (nM != 3) return LFPLUS_E_ARG;      // (ComR1CS: every reference use has M = cr1cs.x.matrices())
    LFP_GUARD(prover_create_impl(device, params, A, seed, n, Lin::r1cs(nM), rowptr, col, val, ncomp, transcript, out), LFPLUS_E_HIP)
}
// ---- the same objects for committed CCS instances: the shape in place of nM
static int create_ccs_impl(int device, const lfplus_params *params, const uint64_t *A, uint64_t seed, uint64_t n, const lfplus_ccs *shape, const uint32_t *const *rowptr,
                           const uint32_t *const *col, const uint64_t *const *val, uint32_t ncomp, lfplus_transcript *transcript, lfplus_prover **out) {
    Lin lin;
    if (!Lin::from_ccs(shape, lin)) return LFPLUS_E_ARG;      // (no context exists yet)
    return prover_create_impl(device, params, A, seed, n, lin, rowptr, col, val, ncomp, transcript, out);
}
extern "C" int lfplus_prover_create_ccs(int device, const lfplus_params *params, const uint64_t *A, uint64_t seed, uint64_t n, const lfplus_ccs *shape, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val, uint32_t ncomp, lfplus_transcript *transcript, lfplus_prover **out) {
    if (!out) return LFPLUS_E_ARG;
    *out = nullptr;
    LFP_GUARD(create_ccs_impl(device, params, A, seed, n, shape, rowptr, col, val, ncomp, transcript, out), LFPLUS_E_HIP)
}
static uint64_t proof_len_ccs_impl(const lfplus_params *p, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh) {
    Lin lin;
    return Lin::from_ccs(shape, lin) ? proof_len_impl(p, n, lin, L, nfresh) : 0;
}
static int proof_layout_ccs_impl(const lfplus_params *p, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh, uint64_t *offsets, uint64_t *lengths, uint32_t nfields) {
    Lin lin;
    return Lin::from_ccs(shape, lin) ? proof_layout_impl(p, n, lin, L, nfresh, offsets, lengths, nfields) : LFPLUS_E_ARG;
}
static int verify_ccs_impl(const lfplus_params *p, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh, lfplus_transcript *tr, const uint64_t *proof,
                           uint64_t proof_words, int *which, int *stage) {
    if (which) *which = -1;
    if (stage) *stage = 0;
    Lin lin;
    return Lin::from_ccs(shape, lin) ? verify_impl(p, n, lin, L, nfresh, tr, proof, proof_words, which, stage) : LFPLUS_E_ARG;
}
extern "C" uint64_t lfplus_proof_len_ccs(const lfplus_params *p, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh) {
    LFP_GUARD(proof_len_ccs_impl(p, n, shape, L, nfresh), 0)
}
extern "C" int lfplus_proof_layout_ccs(const lfplus_params *p, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh, uint64_t *offsets, uint64_t *lengths, uint32_t nfields) {
    LFP_GUARD(proof_layout_ccs_impl(p, n, shape, L, nfresh, offsets, lengths, nfields), LFPLUS_E_HIP)
}
extern "C" int lfplus_verify_ccs(const lfplus_params *p, uint64_t n, const lfplus_ccs *shape, uint32_t L, uint32_t nfresh, lfplus_transcript *tr, const uint64_t *proof, uint64_t proof_words, int *which, int *stage) {
    LFP_GUARD(verify_ccs_impl(p, n, shape, L, nfresh, tr, proof, proof_words, which, stage), LFPLUS_E_HIP)
}
extern "C" int lfplus_prover_check_fresh(lfplus_prover *pr, uint64_t bound, int *ok, unsigned *failed, uint64_t *first_bad, uint64_t *absmax) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_check_fresh_impl(pr, bound, ok, failed, first_bad, absmax), pbreak_nothrow(pr, "lfplus_prover_check_fresh: out of host memory"))
}
extern "C" int lfplus_prover_ingest(lfplus_prover *pr, const uint64_t *const *z, uint32_t count, uint64_t m, uint32_t l_in, uint64_t *cm_f_out) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_ingest_impl(pr, z, count, m, l_in, cm_f_out, Origin::host), pbreak_nothrow(pr, "lfplus_prover_ingest: out of host memory"))
}
extern "C" int lfplus_prover_ingest_dev(lfplus_prover *pr, const uint64_t *const *z, uint32_t count, uint64_t m, uint32_t l_in, uint64_t *cm_f_out) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_ingest_impl(pr, z, count, m, l_in, cm_f_out, Origin::device), pbreak_nothrow(pr, "lfplus_prover_ingest_dev: out of host memory"))
}
extern "C" int lfplus_prover_set_instances(lfplus_prover *pr, const uint64_t *const *f, const uint64_t *const *cm_f, uint32_t count) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_set_instances_impl(pr, f, cm_f, count, Origin::host), pbreak_nothrow(pr, "lfplus_prover_set_instances: out of host memory"))
}
extern "C" int lfplus_prover_set_instances_dev(lfplus_prover *pr, const uint64_t *const *f, const uint64_t *const *cm_f, uint32_t count) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_set_instances_impl(pr, f, cm_f, count, Origin::device), pbreak_nothrow(pr, "lfplus_prover_set_instances_dev: out of host memory"))
}
extern "C" int lfplus_prover_wait_stream(lfplus_prover *pr, void *hip_stream) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_wait_stream_impl(pr, hip_stream), pfail(pr, LFPLUS_E_HIP, "lfplus_prover_wait_stream: out of host memory"))
}
extern "C" int lfplus_prover_prove(lfplus_prover *pr, uint64_t *proof, uint64_t proof_words) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_prove_impl(pr, proof, proof_words), pbreak_nothrow(pr, "lfplus_prover_prove: out of host memory"))
}
extern "C" int lfplus_prover_accumulator(lfplus_prover *pr, uint64_t *F0, uint64_t *F1) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_accumulator_impl(pr, F0, F1, Origin::host), pfail(pr, LFPLUS_E_HIP, "lfplus_prover_accumulator: out of host memory"))
}
extern "C" int lfplus_prover_accumulator_dev(lfplus_prover *pr, uint64_t *F0, uint64_t *F1) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_accumulator_impl(pr, F0, F1, Origin::device), pfail(pr, LFPLUS_E_HIP, "lfplus_prover_accumulator_dev: out of host memory"))
}
extern "C" int lfplus_prover_decide(lfplus_prover *pr, const uint64_t *proof, uint64_t proof_words, uint64_t bound, int *ok, unsigned *failed, uint64_t *absmax) {
    if (!pr) return LFPLUS_E_ARG;
    LFP_GUARD(prover_decide_impl(pr, proof, proof_words, bound, ok, failed, absmax), pfail(pr, LFPLUS_E_HIP, "lfplus_prover_decide: out of host memory"))
}
