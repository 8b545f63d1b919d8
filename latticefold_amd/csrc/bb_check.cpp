// bb_check.cpp -- BabyBear backend: the relation checks of lf_check.cpp (CCS::check_relation arith.rs:76-110, R_CCCS, R_LCCCS arith.rs:193-206) with
// 72-word ring elements and F_{p^9} slots.  The residual kernel is bb_check.hip's; the plane norm is the ring-agnostic lf::launch_planes_absmax.
#include "bb_ctx.h"
#include "lf_check.h"

namespace lfbb {

// M_j z for every matrix j -> mz [t][72][m]
static void mz_tables(C *c, const fe *z, fe *mz) {
    for (u32 j = 0; j < c->P.t; j++) launch_spmv(c->dev, c->d_rowptr[j], c->d_col[j], c->d_val[j], z, c->n, mz + (size_t)j * RE * c->m, c->m, 0, c->stream());
}
// the device words of a check: [0] first bad row (starts at m), [1] largest |plane| (starts at 0)
static int check_words(C *c, u32 *w) {
    HIPCHK(hipMemsetD32Async(w, (int)c->m, 1, c->stream()));
    HIPCHK(hipMemsetAsync(w + 1, 0, 4, c->stream()));
    return LF_OK;
}
static int ccs_residual(C *c, const fe *z, u32 *w) {
    fe *mz;
    RET(c->tbuf("chk_mz", (size_t)c->P.t * RE * c->m, &mz));
    mz_tables(c, z, mz);
    launch_ccs_residual(c->dev, c->desc, mz, c->m, c->m, w, c->stream());
    return LF_OK;
}
static int check_state(C *c, const lf_witness *wit, bool need_A) {
    if (!c->have_ccs) return LF_ERR_STATE;
    if (c->sh_world > 1) return LF_ERR_UNSUPPORTED;
    if (wit && wit->N != c->N) return LF_ERR_INVALID;
    if (need_A && !c->dAb) return LF_ERR_STATE;
    if (need_A && c->nA_total != c->N) return LF_ERR_INVALID;
    return LF_OK;
}
static bool same_words(const u64 *a, const u64 *b, size_t n) { return !memcmp(a, b, n * 8); }

int BbCtx::ccs_check(const uint64_t *z, uint64_t *first_bad) {
    C *c = p;
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, nullptr, false));
    HIPCHK(hipSetDevice(c->device));
    fe *zd;
    u64 *od;
    RET(c->tbuf("chk_z", (size_t)RE * c->n, &zd));
    RET(c->tbuf("chk_od", 8, &od));
    u32 *w = (u32 *)od;
    RET(up_ring(c, z, c->n, zd));
    RET(check_words(c, w));
    RET(ccs_residual(c, zd, w));
    u32 h[2];
    RET(down_small(c, od, 1, (u64 *)h));
    *first_bad = h[0];
    return h[0] < c->m ? LF_ERR_REJECT : LF_OK;
}

int BbCtx::cccs_check(const uint64_t *cccs, const lf_witness *wit, uint64_t bound, unsigned *failed, uint64_t *first_bad) {
    C *c = p;
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, wit, true));
    HIPCHK(hipSetDevice(c->device));
    const lf_params &P = c->P;
    const size_t cmw = (size_t)P.kappa * RE;
    std::vector<u64> head((size_t)(P.l + 1) * RE);   // z = x_ccs || 1 || w_ccs
    memcpy(head.data(), cccs + cmw, (size_t)P.l * RE * 8);
    BbHostRing::from_u64(1, head.data() + (size_t)P.l * RE);
    fe *zd;
    u64 *od;
    RET(c->tbuf("chk_z", (size_t)RE * c->n, &zd));
    RET(c->tbuf("chk_od", cmw + 8, &od));   // cm [kappa][72] | the check words
    u32 *w = (u32 *)(od + cmw);
    RET(check_words(c, w));
    RET(build_z(c, wit->planes, 1, 0, head.data(), zd));
    RET(ccs_residual(c, zd, w));
    if (bound) lf::launch_planes_absmax(wit->planes, (size_t)RE * wit->N, w + 1, c->stream());
    RET(witness_commit_dev(c, wit, od));
    std::vector<u64> h(cmw + 1);
    RET(down_small(c, od, cmw + 1, h.data()));
    u32 hw[2];
    memcpy(hw, &h[cmw], 8);
    unsigned f = 0;
    if (!same_words(h.data(), cccs, cmw)) f |= LF_REL_CM;
    if (hw[0] < c->m) f |= LF_REL_CCS;
    if (bound && hw[1] >= bound) f |= LF_REL_NORM;
    *failed = f;
    *first_bad = hw[0];
    return f ? LF_ERR_REJECT : LF_OK;
}

int BbCtx::lcccs_check(const uint64_t *lcccs, const lf_witness *wit, uint64_t bound, unsigned *failed) {
    C *c = p;
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, wit, true));
    const lf_params &P = c->P;
    std::vector<H9> pt;
    if (!lcccs_point(P, lcccs, pt)) return LF_ERR_UNSUPPORTED;
    HIPCHK(hipSetDevice(c->device));
    // lcccs = r[s] v[9] cm[kappa] u[t] x_w[l] h
    const size_t vw = (size_t)TAU * RE, uw = (size_t)P.t * RE, cmw = (size_t)P.kappa * RE, ou = 0, ov = uw, ocm = ov + vw, ow = ocm + cmw;
    const u64 *v_in = lcccs + (size_t)P.s * RE, *cm_in = v_in + vw, *u_in = cm_in + cmw, *xh = u_in + uw;
    fe *zd, *mz, *eqr;
    i64 *partial;
    u64 *od;
    RET(c->tbuf("chk_z", (size_t)RE * c->n, &zd));
    RET(c->tbuf("chk_mz", (size_t)P.t * RE * c->m, &mz));
    RET(c->tbuf("chk_eq", (size_t)TAU * c->m, &eqr));
    RET(c->tbuf("red_partial", red_partial_words(16 * RE * TAU), &partial));
    RET(c->tbuf("chk_od", ow + 8, &od));   // u [t][72] | v [9][72] | cm [kappa][72] | the check words
    u32 *w = (u32 *)(od + ow);
    RET(check_words(c, w));
    RET(build_z(c, wit->planes, 1, 0, xh, zd));   // z = x_w || h || w_ccs
    mz_tables(c, zd, mz);
    RET(build_eq_dev(c, pt.data(), P.s, eqr));
    launch_dot_eq(c->dev, mz, c->m, P.t, eqr, c->m, c->m, partial, od + ou, c->stream());          // u_j = MLE(M_j z)(r)
    launch_coef_eval(c->dev, wit->planes, c->N, eqr, c->m, 1, 0, partial, od + ov, c->stream());   // v = f-hat(r): T[72][9] == v[9][8][9]
    if (bound) lf::launch_planes_absmax(wit->planes, (size_t)RE * wit->N, w + 1, c->stream());
    RET(witness_commit_dev(c, wit, od + ocm));
    std::vector<u64> h(ow + 1);
    RET(down_small(c, od, ow + 1, h.data()));
    u32 hw[2];
    memcpy(hw, &h[ow], 8);
    unsigned f = 0;
    if (!same_words(h.data() + ocm, cm_in, cmw)) f |= LF_REL_CM;
    if (!same_words(h.data() + ou, u_in, uw)) f |= LF_REL_U;
    if (!same_words(h.data() + ov, v_in, vw)) f |= LF_REL_V;
    if (bound && hw[1] >= bound) f |= LF_REL_NORM;
    *failed = f;
    return f ? LF_ERR_REJECT : LF_OK;
}

}  // namespace lfbb
