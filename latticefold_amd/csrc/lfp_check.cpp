// lfp_check.cpp -- on-device relation checks of the LatticeFold+ slice (include/lfplus.h): lfplus_r1cs_check (R_ComR1CS, r1cs.rs:21-60) and lfplus_linb_check
// (R_LinB, lin.rs:29-40) on the resident (A, f), and lfplus_ccs_check, lfplus_r1cs_check for a CCS shape (lfp_ccs.h).  The reference has no check_relation for these; the relations are the ones its structs define and its tests
// assert piecewise (decomp.rs:157-215, r1cs.rs:211-233).  Kernels: lfp_check.hip.  The calls are read-only: they touch neither the witness, the from_f buffers
// nor a transcript; every component is evaluated and *failed is the OR of the failing ones; the result words come back in ONE download.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/lfplus.h"
#include "lfp_kernels.h"
#include "lfp_ctx.h"
#include "lfp_ccs.h"

namespace {
constexpr int D = lfp::D;
u64 to_mont(u64 a) { return (u64)((((unsigned __int128)a) << 64) % lfp::P); }
// scratch of one call, from the context's pool
struct Scratch {
    lfplus_ctx *c;
    std::vector<void *> held;
    explicit Scratch(lfplus_ctx *c_) : c(c_) {}
    ~Scratch() {      // (an error return may leave work of this call in flight: drain it before the blocks can be handed out again)
        (void)hipStreamSynchronize(c->st);
        for (void *p : held) c->pool.put(p);
    }
    u64 *words(size_t n) {
        void *p = c->pool.get((n ? n : 1) * 8);
        if (p) held.push_back(p);
        return (u64 *)p;
    }
};
// the matrices of one call: the caller's CSR arrays, uploaded (and validated: lfp_upload_matrix) for its duration, or the resident ones (rowptr == NULL)
struct Mats {
    std::vector<LfpMatrix> own;
    const LfpMatrix *m = nullptr;
    ~Mats() { for (LfpMatrix &x : own) x.release(); }
    int get(lfplus_ctx *c, const char *who, u32 nM, const u32 *const *rowptr, const u32 *const *col, const u64 *const *val) {
        if (!nM) return LFPLUS_OK;
        if (!rowptr) {
            if (c->mats.size() != nM || c->mats_n != c->n) return fail(c, LFPLUS_E_ARG, std::string(who) + ": no resident matrices of this number and shape (lfplus_set_matrices)");
            m = c->mats.data();
            return LFPLUS_OK;
        }
        if (!col || !val) return fail(c, LFPLUS_E_ARG, std::string(who) + ": null argument");
        own.resize(nM);
        for (u32 q = 0; q < nM; q++) {
            int rc = lfp_upload_matrix(c, (size_t)c->n, rowptr[q], col[q], val[q], own[q]);
            if (rc) return rc;
        }
        m = own.data();
        return LFPLUS_OK;
    }
};
// what both checks ask of the context; joins a pending lfplus_rg_from_f_async pass
int check_ctx(lfplus_ctx *c, const char *who, const unsigned *failed, const u64 *cm_f) {
    if (!c) return LFPLUS_E_ARG;
    if (!failed) return fail(c, LFPLUS_E_ARG, std::string(who) + ": null argument");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, std::string(who) + ": sharded contexts are not supported (a rank holds only its columns of A)");
    if (!c->A || !c->f || c->nf != c->n) return fail(c, LFPLUS_E_ARG, std::string(who) + ": matrix / witness not set or of different length");
    if (c->n & (c->n - 1)) return fail(c, LFPLUS_E_ARG, std::string(who) + ": n must be a power of two");
    if (cm_f && !canonical(cm_f, (size_t)c->kappa * D)) return fail(c, LFPLUS_E_ARG, std::string(who) + ": non-canonical commitment word");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, LFPLUS_E_HIP, "hipSetDevice");
    return lfplus_join_async(c);
}
// result words of a call on the device: [0] first bad row (starts at n), [1] absmax (starts at 0), [2, 2 + kappa 16) A f, then the evaluations
constexpr size_t RES_HEAD = 2;
int start_result(lfplus_ctx *c, u64 *res, const u64 *init2, const u64 *cm_f) {
    HIPCHK(c, hipMemcpyAsync(res, init2, RES_HEAD * 8, hipMemcpyHostToDevice, c->st));
    if (cm_f) {      // the path of lfplus_commit_resident; compared on the host
        u64 *cm = nullptr;
        int rc = lfp_commit_resident_enqueue(c, &cm);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(res + RES_HEAD, cm, (size_t)c->kappa * D * 8, hipMemcpyDeviceToDevice, c->st));
    }
    return LFPLUS_OK;
}
int finish_result(lfplus_ctx *c, const u64 *res, std::vector<u64> &h) {
    HIPCHK(c, hipMemcpyAsync(h.data(), res, h.size() * 8, hipMemcpyDeviceToHost, c->st));      // the one download
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return LFPLUS_OK;
}
}  // namespace

extern "C" int lfplus_r1cs_check(lfplus_ctx *c, const uint64_t *cm_f, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val,
                                 uint64_t bound, unsigned *failed, uint64_t *first_bad, uint64_t *absmax) {
    int rc = check_ctx(c, "lfplus_r1cs_check", failed, cm_f);
    if (rc) return rc;
    Mats M;
    if ((rc = M.get(c, "lfplus_r1cs_check", 3, rowptr, col, val))) return rc;
    const u64 n = c->n;
    const size_t cw = (size_t)c->kappa * D;
    Scratch sc(c);
    u64 *res = sc.words(RES_HEAD + cw);
    if (!res) return fail(c, LFPLUS_E_HIP, "lfplus_r1cs_check: out of device memory");
    const u64 init2[RES_HEAD] = {n, 0};
    if ((rc = start_result(c, res, init2, cm_f))) return rc;
    const u32 *rp[3], *ci[3];
    const u64 *vv[3];
    int cc[3];
    for (int q = 0; q < 3; q++) { rp[q] = M.m[q].rowptr; ci[q] = M.m[q].col; vv[q] = M.m[q].spmv_vals(); cc[q] = M.m[q].const_coef; }
    lfp::launch_r1cs_residual(rp, ci, vv, cc, c->f, (size_t)n, res, c->st);
    if (absmax || bound) lfp::launch_absmax(c->f, (size_t)n * D, res + 1, c->st);
    std::vector<u64> h(RES_HEAD + cw);
    if ((rc = finish_result(c, res, h))) return rc;
    unsigned bad = 0;
    if (cm_f && memcmp(cm_f, h.data() + RES_HEAD, cw * 8)) bad |= LFPLUS_REL_CM;
    if (h[0] != n) bad |= LFPLUS_REL_R1CS;
    if (bound && !(h[1] < bound)) bad |= LFPLUS_REL_NORM;
    *failed = bad;
    if (first_bad) *first_bad = h[0];
    if (absmax) *absmax = h[1];
    return bad ? fail(c, LFPLUS_E_REJECT, "lfplus_r1cs_check: the instance does not satisfy R_ComR1CS") : LFPLUS_OK;
}

// lfplus_r1cs_check for a CCS shape: cm_f = A f, the norm rule, and sum_i c_i prod_{j in S_i} (M_j f)[row] = 0 row by row (fused: launch_ccs_residual)
extern "C" int lfplus_ccs_check(lfplus_ctx *c, const uint64_t *cm_f, const lfplus_ccs *shape, const uint32_t *const *rowptr, const uint32_t *const *col,
                                const uint64_t *const *val, uint64_t bound, unsigned *failed, uint64_t *first_bad, uint64_t *absmax) {
    if (!c) return LFPLUS_E_ARG;
    lfp::CcsDesc d;
    int rc = lfp_ccs_shape(c, "lfplus_ccs_check", shape, d, nullptr);
    if (rc) return rc;
    if ((rc = check_ctx(c, "lfplus_ccs_check", failed, cm_f))) return rc;
    Mats M;
    if ((rc = M.get(c, "lfplus_ccs_check", d.t, rowptr, col, val))) return rc;
    const u64 n = c->n;
    const size_t cw = (size_t)c->kappa * D;
    Scratch sc(c);
    u64 *res = sc.words(RES_HEAD + cw), *coefM = sc.words((size_t)d.q * D);
    if (!res || !coefM) return fail(c, LFPLUS_E_HIP, "lfplus_ccs_check: out of device memory");
    const u64 init2[RES_HEAD] = {n, 0};
    if ((rc = start_result(c, res, init2, cm_f))) return rc;
    std::vector<u64> hM((size_t)d.q * D);
    for (size_t i = 0; i < hM.size(); i++) hM[i] = to_mont(shape->c[i]);
    HIPCHK(c, hipMemcpyAsync(coefM, hM.data(), hM.size() * 8, hipMemcpyHostToDevice, c->st));
    const u32 *rp[8], *ci[8];
    const u64 *vv[8];
    int cc[8];
    for (u32 q = 0; q < d.t; q++) { rp[q] = M.m[q].rowptr; ci[q] = M.m[q].col; vv[q] = M.m[q].spmv_vals(); cc[q] = M.m[q].const_coef; }
    lfp::launch_ccs_residual(rp, ci, vv, cc, d, coefM, c->f, (size_t)n, res, c->st);
    if (absmax || bound) lfp::launch_absmax(c->f, (size_t)n * D, res + 1, c->st);
    std::vector<u64> h(RES_HEAD + cw);
    if ((rc = finish_result(c, res, h))) return rc;      // (synchronises: hM is free)
    unsigned bad = 0;
    if (cm_f && memcmp(cm_f, h.data() + RES_HEAD, cw * 8)) bad |= LFPLUS_REL_CM;
    if (h[0] != n) bad |= LFPLUS_REL_CCS;
    if (bound && !(h[1] < bound)) bad |= LFPLUS_REL_NORM;
    *failed = bad;
    if (first_bad) *first_bad = h[0];
    if (absmax) *absmax = h[1];
    return bad ? fail(c, LFPLUS_E_REJECT, "lfplus_ccs_check: the instance does not satisfy the committed CCS relation") : LFPLUS_OK;
}

extern "C" int lfplus_linb_check(lfplus_ctx *c, const uint64_t *cm_f, const uint64_t *r_a, const uint64_t *r_b, uint32_t nM, const uint32_t *const *rowptr,
                                 const uint32_t *const *col, const uint64_t *const *val, const uint64_t *v, uint64_t bound, unsigned *failed, uint64_t *absmax) {
    int rc = check_ctx(c, "lfplus_linb_check", failed, cm_f);
    if (rc) return rc;
    if (!r_a || !r_b || !v || nM > 64) return fail(c, LFPLUS_E_ARG, "lfplus_linb_check: null argument / more than 64 matrices");
    const u64 n = c->n;
    u32 nvars = 0;
    while (((u64)1 << nvars) < n) nvars++;
    const u32 T = 2 * (1 + nM);      // evaluations: (f, M_0 f, ..) x (r_a, r_b), index q * 2 + point as in lfplus_decompose's v0
    if (!canonical(r_a, (size_t)nvars * D) || !canonical(r_b, (size_t)nvars * D)) return fail(c, LFPLUS_E_ARG, "lfplus_linb_check: non-canonical point");
    if (!canonical(v, (size_t)T * D)) return fail(c, LFPLUS_E_ARG, "lfplus_linb_check: non-canonical evaluation word");
    Mats M;
    if ((rc = M.get(c, "lfplus_linb_check", nM, rowptr, col, val))) return rc;
    // Scalar path: every coordinate of both points is a ring constant (always, for PlusProver's points) and every matrix has constant coefficients -- then
    // eq(r_pt) and M_j^T eq(r_pt) are SCALAR weight vectors and the evaluations are inner products <f, w>: one pass over f (k_linb_dots).  Otherwise the tables
    // of lfplus_decompose (f and M_j f replicated per point, fix_variables over ring elements): correctness only.
    bool scalar = getenv("LFPLUS_LINB_TABLES") == nullptr;   // (read per call: the tests flip it) the R_LinB check through fix_variables tables even for constant points and coefficients
    for (size_t i = 0; i < (size_t)nvars * D && scalar; i++)
        if (i % D && (r_a[i] || r_b[i])) scalar = false;
    for (u32 j = 0; j < nM && scalar; j++) scalar = M.m[j].const_coef;
    const size_t cw = (size_t)c->kappa * D, vw = (size_t)n * D;
    const bool want_abs = absmax || bound;
    std::vector<u64> rM;      // (declared before the scratch: it outlives the drain of an asynchronous upload from it)
    Scratch sc(c);
    u64 *res = sc.words(RES_HEAD + cw + (size_t)T * D);
    if (!res) return fail(c, LFPLUS_E_HIP, "lfplus_linb_check: out of device memory");
    u64 *ev = res + RES_HEAD + cw;
    const u64 init2[RES_HEAD] = {n, 0};
    if ((rc = start_result(c, res, init2, cm_f))) return rc;
    if (scalar) {
        u64 *W = sc.words((size_t)T * n), *part = sc.words((size_t)lfp::eval_chunks((size_t)n) * 8 * D);
        if (!W || !part) return fail(c, LFPLUS_E_HIP, "lfplus_linb_check: out of device memory");
        for (int pt = 0; pt < 2; pt++) {
            const u64 *r = pt ? r_b : r_a;
            lfp::EqPt e;
            for (u32 j = 0; j < nvars; j++) {
                const u64 x = r[(size_t)j * D];
                e.c[j] = to_mont(x);
                e.nc[j] = to_mont(x <= 1 ? 1 - x : lfp::P + 1 - x);
            }
            e.one = to_mont(1);
            lfp::launch_eq_build(e, nvars, W + (size_t)pt * n, c->st);
            for (u32 j = 0; j < nM; j++)
                lfp::launch_spmvT_eq_const(M.m[j].colptr, M.m[j].rowidx, M.m[j].valTc, W + (size_t)pt * n, (size_t)n, W + ((size_t)(1 + j) * 2 + pt) * n, c->st);
        }
        for (u32 t0 = 0; t0 < T;) {      // eight weight vectors per pass: ONE pass over f for up to three matrices
            const u32 nw = T - t0 >= 8 ? 8 : T - t0 >= 4 ? 4 : 2;
            lfp::launch_linb_dots(c->f, (size_t)n, W + (size_t)t0 * n, (size_t)n, nw, part, ev + (size_t)t0 * D, want_abs && !t0 ? res + 1 : nullptr, c->st);
            t0 += nw;
        }
    } else {
        u64 *tab = sc.words((size_t)T * vw), *ping = sc.words((size_t)T * vw / 2 + D), *drM = sc.words((size_t)nvars * 2 * D + D), *dy = sc.words(vw);
        if (!tab || !ping || !drM || !dy) return fail(c, LFPLUS_E_HIP, "lfplus_linb_check: out of device memory");
        rM.resize((size_t)nvars * 2 * D);
        for (u32 k = 0; k < nvars; k++)
            for (int w = 0; w < D; w++) {
                rM[(size_t)k * 2 * D + w] = to_mont(r_a[(size_t)k * D + w]);
                rM[(size_t)k * 2 * D + D + w] = to_mont(r_b[(size_t)k * D + w]);
            }
        if (nvars) HIPCHK(c, hipMemcpyAsync(drM, rM.data(), rM.size() * 8, hipMemcpyHostToDevice, c->st));
        lfp::launch_replicate(c->f, vw, 2, tab, c->st);
        for (u32 j = 0; j < nM; j++) {
            lfp::launch_spmv_ring(M.m[j].rowptr, M.m[j].col, M.m[j].spmv_vals(), c->f, (size_t)n, dy, c->st, M.m[j].const_coef);
            lfp::launch_replicate(dy, vw, 2, tab + (size_t)(1 + j) * 2 * vw, c->st);
        }
        u64 *cur = tab, *nxt = ping;
        size_t len = (size_t)n;
        for (u32 k = 0; k < nvars; k++) {      // fix_variables, variable 0 first, all T tables at once (table t evaluates at point t & 1)
            bool const_r = true;
            for (int w = 1; w < D && const_r; w++) const_r = !r_a[(size_t)k * D + w] && !r_b[(size_t)k * D + w];
            lfp::launch_ring_fix(cur, nxt, T, len, drM + (size_t)k * 2 * D, c->st, const_r);
            std::swap(cur, nxt);
            len /= 2;
        }
        HIPCHK(c, hipMemcpyAsync(ev, cur, (size_t)T * D * 8, hipMemcpyDeviceToDevice, c->st));
        if (want_abs) lfp::launch_absmax(c->f, vw, res + 1, c->st);
    }
    std::vector<u64> h(RES_HEAD + cw + (size_t)T * D);
    if ((rc = finish_result(c, res, h))) return rc;
    unsigned bad = 0;
    if (cm_f && memcmp(cm_f, h.data() + RES_HEAD, cw * 8)) bad |= LFPLUS_REL_CM;
    if (memcmp(v, h.data() + RES_HEAD + cw, (size_t)T * D * 8)) bad |= LFPLUS_REL_V;
    if (bound && !(h[1] < bound)) bad |= LFPLUS_REL_NORM;
    *failed = bad;
    if (absmax) *absmax = h[1];
    return bad ? fail(c, LFPLUS_E_REJECT, "lfplus_linb_check: the instance does not satisfy R_LinB") : LFPLUS_OK;
}
