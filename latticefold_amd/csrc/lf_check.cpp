// lf_check.cpp -- relation checks on the device (include/lfhip.h "relation checks"): CCS::check_relation (arith.rs:76-110), R_CCCS and R_LCCCS -- the
// decider of an accumulator (arith.rs:193-206).  Goldilocks here; BabyBear contexts forward to BbCtx (bb_check.cpp).
//
// Every piece but the residual is an existing launcher: z from the witness planes (build_z: launch_recompose_crt), M_j z (launch_spmv /
// launch_spmv_rows, the tables [t][24][m] the linearization builds), u = <M_j z, eq(r)> (launch_dot_eq), v = f-hat(r) from the planes (launch_coef_eval),
// cm = Witness::commit (the int8 general commit).  New: the residual with its first-bad-row reduction and the plane norm (lf_check.hip).  Every
// component is evaluated and the small results come back in ONE download.
#include "lf_check.h"
#include "lf_ctx.h"

// M_j z for every matrix j -> mz [t][24][m] (z [24][n] on the device); both CSR layouts, as in the linearization
static int mz_tables(lf_ctx *c, const u64 *z, u64 *mz) {
    const lf_params &P = c->P;
    if (c->ccs_general) {
        u64 *zaos;
        RET(c->tbuf("spmv_zaos", (size_t)P.t * c->n * 24, &zaos));
        launch_soa_to_aos(z, zaos, c->n, c->stream());
        for (u32 j = 0; j < P.t; j++)
            launch_spmv_rows(c->dcrt, 1, &c->d_rowptr[j], &c->d_col[j], &c->d_val[j], nullptr, 0, c->n, zaos, mz + (size_t)j * 24 * c->m, c->m, 0, c->stream());
    } else
        for (u32 j = 0; j < P.t; j++) launch_spmv(c->dcrt, c->d_rowptr[j], c->d_col[j], c->d_val[j], z, c->n, mz + (size_t)j * 24 * c->m, c->m, 0, c->stream());
    return LF_OK;
}

// the device words of a check: [0] first bad row (starts at m), [1] largest |plane| (starts at 0)
static int check_words(lf_ctx *c, u32 *w) {
    HIPCHK(hipMemsetD32Async(w, (int)c->m, 1, c->stream()));
    HIPCHK(hipMemsetAsync(w + 1, 0, 4, c->stream()));
    return LF_OK;
}

// z -> M_j z -> residual: lowers w[0] to the first bad row
static int ccs_residual(lf_ctx *c, const u64 *z, u32 *w) {
    u64 *mz;
    RET(c->tbuf("chk_mz", (size_t)c->P.t * 24 * c->m, &mz));
    RET(mz_tables(c, z, mz));
    launch_ccs_residual(c->dcrt, c->desc, mz, c->m, c->m, w, c->stream());
    return LF_OK;
}

static int check_state(lf_ctx *c, const lf_witness *wit, bool need_A) {
    if (!c->have_ccs) return LF_ERR_STATE;
    if (c->sh_world > 1) return LF_ERR_UNSUPPORTED;   // sharded deciding is not implemented
    if (wit && wit->N != c->N) return LF_ERR_INVALID;
    if (need_A && !c->A_loaded) return LF_ERR_STATE;
    if (need_A && c->nA_total != c->N) return LF_ERR_INVALID;   // CommitmentError::WrongWitnessLength
    return LF_OK;
}

static bool same_words(const u64 *a, const u64 *b, size_t n) { return !memcmp(a, b, n * 8); }

int lf_ccs_check(lf_ctx *c, const uint64_t *z, uint64_t *first_bad) {
    if (LF_XB(c) && z && first_bad && c->have_ccs_any()) { XB x(c); return lf_ccs_check(c, x.ring_in(z, c->n_any()), first_bad); }
    if (!c || !z || !first_bad) return LF_ERR_INVALID;
    if (c->bb) return c->bb->ccs_check(z, first_bad);
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, nullptr, false));
    HIPCHK(hipSetDevice(c->device));
    u64 *zd, *od;
    RET(c->tbuf("chk_z", 24 * c->n, &zd));
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

int lf_cccs_check(lf_ctx *c, const uint64_t *cccs, const lf_witness *wit, uint64_t bound, unsigned *failed, uint64_t *first_bad) {
    if (LF_XB(c) && cccs && c->have_ccs_any()) {
        XB x(c);
        return lf_cccs_check(c, x.ring_in(cccs, lf_cccs_len_ring(&c->params_any(), lf_ctx_ring(c))), wit, bound, failed, first_bad);
    }
    if (!c || !cccs || !wit || !failed || !first_bad || wit->ctx != c) return LF_ERR_INVALID;
    if (c->bb) return c->bb->cccs_check(cccs, wit, bound, failed, first_bad);
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, wit, true));
    HIPCHK(hipSetDevice(c->device));
    const lf_params &P = c->P;
    const size_t cmw = (size_t)P.kappa * 24;
    std::vector<u64> head((size_t)(P.l + 1) * 24);   // z = x_ccs || 1 || w_ccs (arith.rs:399-409)
    memcpy(head.data(), cccs + cmw, (size_t)P.l * 24 * 8);
    HostRing::from_u64(1, head.data() + (size_t)P.l * 24);
    u64 *zd, *od;
    RET(c->tbuf("chk_z", 24 * c->n, &zd));
    RET(c->tbuf("chk_od", cmw + 8, &od));   // cm [kappa][24] | the check words
    u32 *w = (u32 *)(od + cmw);
    RET(check_words(c, w));
    RET(build_z(c, wit->planes, 1, 0, head.data(), zd));
    RET(ccs_residual(c, zd, w));
    if (bound) launch_planes_absmax(wit->planes, (size_t)24 * wit->N, w + 1, c->stream());
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

int lf_lcccs_check(lf_ctx *c, const uint64_t *lcccs, const lf_witness *wit, uint64_t bound, unsigned *failed) {
    if (LF_XB(c) && lcccs && c->have_ccs_any()) {
        XB x(c);
        return lf_lcccs_check(c, x.ring_in(lcccs, lf_lcccs_len_ring(&c->params_any(), lf_ctx_ring(c))), wit, bound, failed);
    }
    if (!c || !lcccs || !wit || !failed || wit->ctx != c) return LF_ERR_INVALID;
    if (c->bb) return c->bb->lcccs_check(lcccs, wit, bound, failed);
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, wit, true));
    const lf_params &P = c->P;
    std::vector<Fq3> pt;
    if (!lcccs_point(P, lcccs, pt)) return LF_ERR_UNSUPPORTED;   // the reference's points are diagonal challenges (as lf_fold_step)
    HIPCHK(hipSetDevice(c->device));
    // lcccs = r[s] v[3] cm[kappa] u[t] x_w[l] h
    const u64 *v_in = lcccs + (size_t)P.s * 24, *cm_in = v_in + 72, *u_in = cm_in + (size_t)P.kappa * 24, *xh = u_in + (size_t)P.t * 24;
    const size_t uw = (size_t)P.t * 24, cmw = (size_t)P.kappa * 24, ou = 0, ov = uw, ocm = ov + 72, ow = ocm + cmw;
    u64 *zd, *mz, *eqr, *partial, *od;
    RET(c->tbuf("chk_z", 24 * c->n, &zd));
    RET(c->tbuf("chk_mz", (size_t)P.t * 24 * c->m, &mz));
    RET(c->tbuf("chk_eq", 3 * c->m, &eqr));
    RET(c->tbuf("red_partial", 256 * 4096, &partial));
    RET(c->tbuf("chk_od", ow + 8, &od));   // u [t][24] | v [3][24] | cm [kappa][24] | the check words
    u32 *w = (u32 *)(od + ow);
    RET(check_words(c, w));
    RET(build_z(c, wit->planes, 1, 0, xh, zd));   // z = x_w || h || w_ccs
    RET(mz_tables(c, zd, mz));
    RET(build_eq_dev(c, pt.data(), P.s, eqr));
    launch_dot_eq(c->dcrt, mz, c->m, P.t, eqr, c->m, c->m, partial, od + ou, c->stream());          // u_j = MLE(M_j z)(r)
    launch_coef_eval(c->dcrt, wit->planes, c->N, eqr, c->m, 1, 0, partial, od + ov, c->stream());   // v = f-hat(r): T[24][3] == v[3][8][3]
    if (bound) launch_planes_absmax(wit->planes, (size_t)24 * wit->N, w + 1, c->stream());
    RET(witness_commit_dev(c, wit, od + ocm));
    std::vector<u64> h(ow + 1);
    RET(down_small(c, od, ow + 1, h.data()));
    u32 hw[2];
    memcpy(hw, &h[ow], 8);
    unsigned f = 0;
    if (!same_words(h.data() + ocm, cm_in, cmw)) f |= LF_REL_CM;
    if (!same_words(h.data() + ou, u_in, uw)) f |= LF_REL_U;
    if (!same_words(h.data() + ov, v_in, 72)) f |= LF_REL_V;
    if (bound && hw[1] >= bound) f |= LF_REL_NORM;
    *failed = f;
    return f ? LF_ERR_REJECT : LF_OK;
}
