// lf_check.cpp -- relation checks on the device (include/lfhip.h "relation checks"): CCS::check_relation (arith.rs:76-110), R_CCCS and R_LCCCS -- the
// decider of an accumulator (arith.rs:193-206).  One body per check for both rings (lf_ring_host.h); the residual kernels are lf_check.hip / bb_check.hip.
//
// Every piece but the residual is an existing launcher: z from the witness planes (build_z: launch_recompose_crt), M_j z (launch_spmv /
// launch_spmv_rows, the tables [t][RE][m] the linearization builds), u = <M_j z, eq(r)> (launch_dot_eq), v = f-hat(r) from the planes (launch_coef_eval),
// cm = Witness::commit (the int8 general commit).  New: the residual with its first-bad-row reduction and the plane norm.  Every
// component is evaluated and the small results come back in ONE download.
#include "lf_ring_host.h"

namespace lfring {

// M_j z for every matrix j -> a fresh mz [t][RE][m] (z [RE][n] on the device).  z_aos (optional, rings with general CSR rows): an element-major z [n][RE] that
// exists already -- the device buffer of an lf_ccs_check_dev caller -- so none is rebuilt
template <class C>
static int mz_tables(C *c, const typename Ring<C>::W *z, typename Ring<C>::W **mz_out, const u64 *z_aos = nullptr) {
    typedef Ring<C> R;
    const lf_params &P = c->P;
    typename R::W *mz;
    RET(c->tbuf("chk_mz", (size_t)P.t * R::RE * c->m, &mz));
    *mz_out = mz;
    if constexpr (R::general_csr) {   // Goldilocks only: both CSR layouts, as in the linearization
        if (c->ccs_general) {
            typename R::W *zaos = (typename R::W *)z_aos;   // (canonical words are this ring's device form)
            if (!zaos) {
                RET(c->tbuf("spmv_zaos", (size_t)P.t * c->n * R::RE, &zaos));
                launch_soa_to_aos(z, zaos, c->n, c->stream());
            }
            for (u32 j = 0; j < P.t; j++)
                launch_spmv_rows(R::tab(c), 1, &c->d_rowptr[j], &c->d_col[j], &c->d_val[j], nullptr, 0, c->n, zaos, mz + (size_t)j * R::RE * c->m, c->m, 0, c->stream());
            return LF_OK;
        }
    }
    for (u32 j = 0; j < P.t; j++) launch_spmv(R::tab(c), c->d_rowptr[j], c->d_col[j], c->d_val[j], z, c->n, mz + (size_t)j * R::RE * c->m, c->m, 0, c->stream());
    return LF_OK;
}

// the device words of a check: [0] first bad row (starts at m), [1] largest |plane| (starts at 0)
template <class C>
static int check_words(C *c, u32 *w) {
    HIPCHK(hipMemsetD32Async(w, (int)c->m, 1, c->stream()));
    HIPCHK(hipMemsetAsync(w + 1, 0, 4, c->stream()));
    return LF_OK;
}

// z -> M_j z -> residual: lowers w[0] to the first bad row
template <class C>
static int ccs_residual(C *c, const typename Ring<C>::W *z, u32 *w, const u64 *z_aos = nullptr) {
    typename Ring<C>::W *mz;
    RET(mz_tables(c, z, &mz, z_aos));
    launch_ccs_residual(Ring<C>::tab(c), c->desc, mz, c->m, c->m, w, c->stream());
    return LF_OK;
}

template <class C>
static int check_state(C *c, const lf_witness *wit, bool need_A) {
    if (!c->have_ccs) return LF_ERR_STATE;
    if (c->sh_world > 1) return LF_ERR_UNSUPPORTED;   // sharded deciding is not implemented
    if (wit && wit->N != c->N) return LF_ERR_INVALID;
    if (need_A && !c->A_loaded) return LF_ERR_STATE;
    if (need_A && c->nA_total != c->N) return LF_ERR_INVALID;   // CommitmentError::WrongWitnessLength
    return LF_OK;
}

static bool same_words(const u64 *a, const u64 *b, size_t n) { return !memcmp(a, b, n * 8); }

template <class C>
static int ccs_check(C *c, const u64 *z, u64 *first_bad, Origin org) {
    typedef Ring<C> R;
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, nullptr, false));
    HIPCHK(hipSetDevice(c->device));
    DevIo<C> io(c, org);
    RET(io.array(z, c->n));
    typename R::W *zd;
    u64 *od;
    RET(c->tbuf("chk_z", (size_t)R::RE * c->n, &zd));
    RET(c->tbuf("chk_od", 8, &od));
    u32 *w = (u32 *)od;
    RET(io.begin());
    RET(up_ring(io, z, c->n, zd, Form::ntt));
    RET(check_words(c, w));
    // a device z is the element-major copy the general CSR rows gather from -- unless it is in an external basis: then the copy is rebuilt from the converted planes
    RET(ccs_residual(c, zd, w, io.dev && !xb_converts(c, Form::ntt) ? z : nullptr));
    u32 h[2];
    RET(io.fetch());                                     // (travels with the download of the check words)
    RET(down_small(c, od, 1, (u64 *)h));
    if (io.bad()) return LF_ERR_INVALID;
    *first_bad = h[0];
    return h[0] < c->m ? LF_ERR_REJECT : LF_OK;
}

template <class C>
static int cccs_check(C *c, const u64 *cccs, const lf_witness *wit, u64 bound, unsigned *failed, u64 *first_bad) {
    typedef Ring<C> R;
    constexpr size_t RE = R::RE;
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, wit, true));
    c->tn = Tunables::read(R::lut_min_default);   // (the commitment's switches, as every entry point that reaches the commit kernels)
    HIPCHK(hipSetDevice(c->device));
    const lf_params &P = c->P;
    const size_t cmw = (size_t)P.kappa * RE;
    std::vector<u64> head((size_t)(P.l + 1) * RE);   // z = x_ccs || 1 || w_ccs (arith.rs:399-409)
    memcpy(head.data(), cccs + cmw, (size_t)P.l * RE * 8);
    decltype(c->ring)::from_u64(1, head.data() + (size_t)P.l * RE);
    typename R::W *zd;
    u64 *od;
    RET(c->tbuf("chk_z", RE * c->n, &zd));
    RET(c->tbuf("chk_od", cmw + 8, &od));   // cm [kappa][RE] | the check words
    u32 *w = (u32 *)(od + cmw);
    RET(check_words(c, w));
    RET(build_z(c, wit->planes, 1, 0, head.data(), zd));
    RET(ccs_residual(c, zd, w));
    if (bound) launch_planes_absmax(wit->planes, RE * wit->N, w + 1, c->stream());
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

template <class C>
static int lcccs_check(C *c, const u64 *lcccs, const lf_witness *wit, u64 bound, unsigned *failed) {
    typedef Ring<C> R;
    constexpr size_t RE = R::RE, TAU = R::TAU;
    std::lock_guard<std::mutex> g(c->mu);
    RET(check_state(c, wit, true));
    c->tn = Tunables::read(R::lut_min_default);   // (the commitment's switches, as every entry point that reaches the commit kernels)
    const lf_params &P = c->P;
    std::vector<typename R::Ext> pt;
    if (!lfs::lcccs_point<typename R::Host>(P, lcccs, pt)) return LF_ERR_UNSUPPORTED;   // the reference's points are diagonal challenges (as lf_fold_step)
    HIPCHK(hipSetDevice(c->device));
    // lcccs = r[s] v[tau] cm[kappa] u[t] x_w[l] h
    const size_t vw = TAU * RE, uw = (size_t)P.t * RE, cmw = (size_t)P.kappa * RE, ou = 0, ov = uw, ocm = ov + vw, ow = ocm + cmw;
    const u64 *v_in = lcccs + (size_t)P.s * RE, *cm_in = v_in + vw, *u_in = cm_in + cmw, *xh = u_in + uw;
    typename R::W *zd, *mz, *eqr;
    typename R::Part *partial;
    u64 *od;
    RET(c->tbuf("chk_z", RE * c->n, &zd));
    RET(c->tbuf("chk_eq", TAU * c->m, &eqr));
    RET(c->tbuf("red_partial", R::red_partial(0), &partial));
    RET(c->tbuf("chk_od", ow + 8, &od));   // u [t][RE] | v [tau][RE] | cm [kappa][RE] | the check words
    u32 *w = (u32 *)(od + ow);
    RET(check_words(c, w));
    RET(build_z(c, wit->planes, 1, 0, xh, zd));   // z = x_w || h || w_ccs
    RET(mz_tables(c, zd, &mz));
    RET(build_eq_dev(c, pt.data(), P.s, eqr));
    launch_dot_eq(R::tab(c), mz, c->m, P.t, eqr, c->m, c->m, partial, od + ou, c->stream());          // u_j = MLE(M_j z)(r)
    launch_coef_eval(R::tab(c), wit->planes, c->N, eqr, c->m, 1, 0, partial, od + ov, c->stream());   // v = f-hat(r): T[RE][tau] == v[tau][8][tau]
    if (bound) launch_planes_absmax(wit->planes, RE * wit->N, w + 1, c->stream());
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

}  // namespace lfring

int lf_ccs_check(lf_ctx *c, const uint64_t *z, uint64_t *first_bad) {
    XbArrays xa(c);
    if (!c || !z || !first_bad) return LF_ERR_INVALID;
    return c->bb ? lfring::ccs_check(c->bb->p, z, first_bad, Origin::host) : lfring::ccs_check(c, z, first_bad, Origin::host);
}
int lf_ccs_check_dev(lf_ctx *c, const uint64_t *z, uint64_t *first_bad) {
    if (!c || !z || !first_bad) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? lfring::ccs_check(c->bb->p, z, first_bad, Origin::device) : lfring::ccs_check(c, z, first_bad, Origin::device);
}

int lf_cccs_check(lf_ctx *c, const uint64_t *cccs, const lf_witness *wit, uint64_t bound, unsigned *failed, uint64_t *first_bad) {
    if (LF_XB(c) && cccs && c->have_ccs_any()) {
        XB x(c);
        return lf_cccs_check(c, x.ring_in(cccs, lf_cccs_len_ring(&c->params_any(), lf_ctx_ring(c))), wit, bound, failed, first_bad);
    }
    if (!c || !cccs || !wit || !failed || !first_bad || wit->ctx != c) return LF_ERR_INVALID;
    return c->bb ? lfring::cccs_check(c->bb->p, cccs, wit, bound, failed, first_bad) : lfring::cccs_check(c, cccs, wit, bound, failed, first_bad);
}

int lf_lcccs_check(lf_ctx *c, const uint64_t *lcccs, const lf_witness *wit, uint64_t bound, unsigned *failed) {
    if (LF_XB(c) && lcccs && c->have_ccs_any()) {
        XB x(c);
        return lf_lcccs_check(c, x.ring_in(lcccs, lf_lcccs_len_ring(&c->params_any(), lf_ctx_ring(c))), wit, bound, failed);
    }
    if (!c || !lcccs || !wit || !failed || wit->ctx != c) return LF_ERR_INVALID;
    return c->bb ? lfring::lcccs_check(c->bb->p, lcccs, wit, bound, failed) : lfring::lcccs_check(c, lcccs, wit, bound, failed);
}
