// lf_ring_host.h -- the host side of the ring-generic entry points, ONCE for both rings (the pattern of poseidon_host.h): a small policy per ring
// (GoldRing: lf_ctx, 24 canonical u64 words, tau 3; BbRing: lfbb::BbCtxImpl, 72 centred Montgomery int32 words, tau 9) and one template per body.
// The launchers are NOT wrapped: lf:: and lfbb:: declare them as overload sets over the word type and the table struct, and both namespaces are
// visible below, so a call resolves by the types the policy hands out.  Context members that carry the same name on both rings (mu, device, stream(),
// tbuf, ring, d_icrt, P, N, m, n, kappa, nA, ...) are used directly.  lf_capi.cpp keeps the argument checks, the external-basis wrapper and the
// dispatch `c->bb ? ring_ops<BbRing>::f(c->bb->p, ..) : ring_ops<GoldRing>::f(c, ..)`.
//
// The context members both rings share are defined once, in lf_ctx_core.h; the set-up bodies (ICRT upload, matrix install, constraint-system load), the general
// commits and the read-outs below use nothing else.
//
// Stays per backend, one line each:
//   build_eq_dev / build_eq_async   two-level kernel on Goldilocks, pre-multiplied constants staged in the pinned arena on BabyBear
//   build_z                         different table layouts (atl() leading dimension)
//   the table build of install_tables, the envelope check of ccs_load   per-ring tables and per-ring limits (wide CCS, small bases on Goldilocks only)
//   down_small                      lane_sync() on a blocking event (Goldilocks) against a plain stream synchronise
//   selftest_field, set_sharding / dist_init   different kernels; two communicators and a handshake against one
//   the SCHEDULES of the provers (lf_prove.cpp, lf_fold.cpp, lf_fold_sb.cpp: lane worker, mailbox tails, sharded rounds, small bases, wide CCS; bb_prove.cpp:
//   one thread, pinned arenas) -- what they enqueue, wait for and time.  The protocol's host arithmetic underneath them (sumcheck transcript, public input,
//   x_s, y_0, the absorbs, the challenge draws, get_rhos, the folded instance, the C_pi table) is lf_step_host.h, shared with the verifier (lf_verify.h), over
//   the host policies GoldV (lf_host.h) / BbV (bb_host.h) -- Ring<Ctx>::Host below
//   lf_dist.cpp, the checks of the verifier, the wire format and lfp_*
//
// Order of the argument checks, the same on both rings: (1) null / range checks of the ABI function -> LF_ERR_INVALID, (2) here, before the context
// lock: pow2(base) -> LF_ERR_UNSUPPORTED (decompose), len against 2^nv -> LF_ERR_INVALID (mle_eval_batch), (3) under the lock: have_ccs / resident
// matrix -> LF_ERR_STATE, then index and length checks -> LF_ERR_INVALID.
#pragma once
#include "bb_ctx.h"
#include "lf_check.h"
#include "lf_ctx.h"
#include "lf_dev_ptr.h"
#include "lf_mlsumcheck.h"
#include "lf_witness_parts.h"

#pragma GCC visibility push(hidden)
// ---- lengths in ring elements (tau = extension degree: the v part of an LCCCS and of the proofs is tau elements) ------------------------------------
inline size_t lcccs_len(const lf_params *p, size_t tau) { return (size_t)p->s + tau + p->kappa + p->t + p->l + 1; }
inline size_t cccs_len(const lf_params *p) { return (size_t)p->kappa + p->l; }
inline size_t lin_proof_len(const lf_params *p, size_t tau) { return (size_t)p->s * (p->d + 2) + tau + p->t; }
inline size_t dec_proof_len(const lf_params *p, size_t tau) { return (size_t)p->K * (p->t + tau + p->l + 1 + p->kappa); }
inline size_t fold_proof_len(const lf_params *p, size_t tau) { return (size_t)p->s * (2 * p->b + 1) + 2 * (size_t)p->K * (tau + p->t); }
inline size_t proof_len(const lf_params *p, size_t tau) { return lin_proof_len(p, tau) + 2 * dec_proof_len(p, tau) + fold_proof_len(p, tau); }

namespace lfring {
using namespace lf;
using namespace lfbb;   // (RE, TAU, D exist in both: always R::RE, R::TAU below -- an unqualified use does not compile)

template <class Ctx> struct Ring;
template <> struct Ring<lf_ctx> {
    typedef u64 W;            // device word: canonical
    typedef u64 Part;         // block partials of the reductions
    typedef Fq3 Ext;
    typedef Fq3Const ExtC;
    typedef GoldV Host;       // host arithmetic of lf_step_host.h
    static constexpr int RE = 24, TAU = 3;
    static constexpr bool general_csr = true;    // ccs_general / launch_spmv_rows exist on this ring only
    static constexpr bool montgomery = false;
    static constexpr u32 max_kappa = 128;        // rows of a resident matrix
    static constexpr size_t lut_min_default = (size_t)1 << 14;   // Tunables::read: this ring's default of LF_FOLD_LUT_MIN
    static constexpr u64 modulus = LF_P;
    static constexpr const char *io_out = "io_b", *i8g_co = "i8g_coef";
    static const DevCrt &tab(const lf_ctx *c) { return c->dcrt; }
    static W from_canon(u64 w) { return w; }
    static XbMat3 xb_mat(const W *m) { XbMat3 r; memcpy(r.m, m, sizeof(r.m)); return r; }   // lf_set_ext_basis: T or T^-1 as a kernel argument
    static void ring_from_u64(u64 v, u64 *o) { HostRing::from_u64(v, o); }
    // the bit-plane form of the witness `planes` belong to, if the running fold step built it for its GEMM rounds (lf_sv_rounds.h): the digit-plane commit
    // kernel then cuts the digits from it.  Null otherwise
    static int bit_planes(lf_ctx *c, const int32_t *planes, const lf_witness *wit, const u32 **bits) {
        *bits = nullptr;
        if (wit && c->A_col0 == 0 && planes == wit->planes && c->nA == c->N)
            for (int sd = 0; sd < 2; sd++)
                if (c->bits_wit[sd] == wit && c->bits_ptr[sd]) {
                    *bits = c->bits_ptr[sd];
                    if (c->stream() != c->st_lane[1]) HIPCHK(hipStreamWaitEvent(c->stream(), c->bits_ev[sd], 0));
                    break;
                }
        return LF_OK;
    }
    // the sumcheck ABI (lf_sumcheck_{lin,fold}_*): leading dimension of a halved table, block partials and message words of a round, the fix launcher
    typedef FoldRoundArgs FoldA;
    static constexpr bool small_base = true;     // b = 4, 8, 16 (lf_sb.h) exist on this ring only
    static constexpr const char *sf_mu = "sf_mu";
    static constexpr size_t lin_out_words = 9 * 24;   // d + 2 <= 9 evaluations
    static size_t halved_ld(size_t n) { return n ? n : 1; }
    static size_t lin_partial_words(size_t) { return round_partial_words(); }
    static size_t fold_partial_words(size_t) { return round_partial_words(); }
    static void fix(lf_ctx *c, const u64 *in, size_t ld_in, u64 *out, size_t ld_out, size_t n_in, u32 rows, const ExtC &r) {
        launch_fix_many(c->dcrt, in, ld_in, out, ld_out, n_in, rows, r, c->stream());
    }
    // the generic sumcheck (lf_mlsumcheck.h): points a block of its round kernel evaluates; the last fix of `rows` extension-field rows of two entries
    // (leading dimension 2) -> canonical words [rows][TAU]
    static constexpr u32 ml_pts = lfml::PTS_GOLD;
    static void fix_final(lf_ctx *c, const u64 *in, size_t, u32 rows, const ExtC &r, u64 *out) { launch_fix_final(c->dcrt, in, rows, r, out, c->stream()); }
    // one row of A (NTT form [RE][cnt]) -> row i of a row chunk of the byte planes: inverse CRT and packing fused
    static int pack_row(lf_ctx *c, const u64 *row, size_t cnt, u32 i, u32 MT, unsigned char *Ab) {
        return launch_ajtai_icrt_pack_i8(c->d_icrt, row, cnt, i, MT, Ab, c->stream()) < 0 ? LF_ERR_HIP : LF_OK;
    }
    static lf_ctx *owner(lf_ctx *c) { return c; }
    static AjtaiI8Ring i8() { return ajtai_i8_goldilocks(); }
    static Ext ext_load(const u64 *w) { return fq3_make(w[0], w[1], w[2]); }
    static ExtC ext_const(const lf_ctx *, const Ext &a) { return f3c(a); }
    static Ext ext_mul(const lf_ctx *c, const Ext &a, const Ext &b) { return c->ring.mul3(a, b); }
    static u64 canon(W w) { return w; }
    static size_t red_partial(size_t nv) { return 256 * (nv > 4096 ? nv : 4096); }
    static int h2d_consts(lf_ctx *c, void *dst, const void *src, size_t bytes) { return c->h2d_small(dst, src, bytes); }   // pinned ring, no synchronisation
    static int commit_finish(lf_ctx *c, u64 *dev, size_t words, u64 *host) { return commit_download(c, dev, words, host); }   // sharded: gathered on the device
};
template <> struct Ring<BbCtxImpl> {
    typedef fe W;             // device word: centred Montgomery int32
    typedef i64 Part;
    typedef H9 Ext;
    typedef E9PreC ExtC;
    typedef BbV Host;
    static constexpr int RE = lfbb::RE, TAU = lfbb::TAU;
    static constexpr bool general_csr = false;
    static constexpr bool montgomery = true;
    static constexpr u32 max_kappa = 32;
    static constexpr size_t lut_min_default = (size_t)1 << 15;
    static constexpr u64 modulus = BB_P;
    static constexpr const char *io_out = "io_o", *i8g_co = "i8g_co";
    static const DevBb &tab(const BbCtxImpl *c) { return c->dev; }
    static W from_canon(u64 w) { return lfbb::from_canon(w); }
    static XbMat9 xb_mat(const W *m) { XbMat9 r; memcpy(r.m, m, sizeof(r.m)); return r; }
    static void ring_from_u64(u64 v, u64 *o) { BbHostRing::from_u64(v, o); }
    static int bit_planes(BbCtxImpl *, const int32_t *, const lf_witness *, const u32 **bits) { *bits = nullptr; return LF_OK; }   // no bit-plane form on this ring
    typedef FoldArgs FoldA;
    static constexpr bool small_base = false;
    static constexpr const char *sf_mu = "sf_mup";
    static constexpr size_t lin_out_words = 5 * RE;
    static size_t halved_ld(size_t n) { return n < 2 ? 2 : n; }   // leading dimensions stay even (8-byte pair loads)
    static size_t lin_partial_words(size_t) { return red_partial_words(5 * RE); }
    static size_t fold_partial_words(size_t m) { return lfbb::fold_partial_words(m); }
    static void fix(BbCtxImpl *c, const fe *in, size_t ld_in, fe *out, size_t ld_out, size_t n_in, u32 rows, const ExtC &r) {
        launch_fix(c->dev, in, ld_in, out, ld_out, n_in, rows, r, c->stream());
    }
    static constexpr u32 ml_pts = lfml::PTS_BB;
    static void fix_final(BbCtxImpl *c, const fe *in, size_t ld_in, u32 rows, const ExtC &r, u64 *out) { launch_fix_final(c->dev, in, ld_in, rows, r, out, c->stream()); }
    static int pack_row(BbCtxImpl *c, const fe *row, size_t cnt, u32 i, u32 MT, unsigned char *Ab) {   // inverse CRT -> canonical element-major words -> bytes
        const AjtaiI8Ring I = i8();
        fe *coef;
        u64 *canon;
        RET(c->tbuf("i8_prep_coef", (size_t)RE * cnt, &coef));
        RET(c->tbuf("i8_prep_canon", (size_t)RE * cnt, &canon));
        launch_icrt_dense(c->d_icrt, row, coef, cnt, c->stream());
        launch_soa_to_aos(coef, canon, cnt, c->stream());
        return launch_ajtai_pack_i8(canon, 1, RE, cnt, i, MT, I.RD, I.NL, Ab, c->stream()) < 0 ? LF_ERR_HIP : LF_OK;
    }
    static lf_ctx *owner(BbCtxImpl *c) { return c->owner; }
    static AjtaiI8Ring i8() { return ajtai_i8_babybear(); }
    static Ext ext_load(const u64 *w) { return h9_load(w); }
    static ExtC ext_const(const BbCtxImpl *c, const Ext &a) { return e9pre_from_h9(a, c->ring.T.nu); }
    static Ext ext_mul(const BbCtxImpl *c, const Ext &a, const Ext &b) { return c->ring.mul9(a, b); }
    static u64 canon(W w) { return to_canon(w); }
    static size_t red_partial(size_t nv) { return red_partial_words((u32)(nv > (size_t)16 * RE * TAU ? nv : (size_t)16 * RE * TAU)); }
    static int h2d_consts(BbCtxImpl *c, void *dst, const void *src, size_t bytes) {   // pageable source: the copy is complete on return
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream()));
        HIPCHK(hipStreamSynchronize(c->stream()));
        return LF_OK;
    }
    static int commit_finish(BbCtxImpl *c, u64 *dev, size_t words, u64 *host) {   // sharded: gathered on the host
        RET(down_small(c, dev, words, host));
        return exchange_modsum(c, host, words);
    }
};
typedef Ring<lf_ctx> GoldRing;
typedef Ring<BbCtxImpl> BbRing;

// ---- host<->device staging of AoS ring-element arrays (canonical u64 at the ABI) ---------------------------------------------------------------------
// What the words of an array at the ABI are: Form::ntt -- NTT-form ring elements, eight slots of F_{p^tau}, presented in the context's external basis
// (lf_set_ext_basis) -- or Form::coeff -- coefficients (lf_decompose / lf_recompose, f_coeff, the input of commit_coeff), which no basis touches.  On a context
// in an external basis an NTT-form array of an entry point that converts (t_xb_arrays, lf_ctx.h) goes through the basis-changing relayout kernels; every other
// array, and every array of a context in the default basis, goes through the plain ones.
enum class Form { ntt, coeff };
template <class C>
inline bool xb_converts(const C *c, Form f) { return f == Form::ntt && c->xb_on && t_xb_arrays; }
// upload n ring elements (AoS) into a plane table dst [RE][n]
template <class C>
int up_ring(C *c, const u64 *host, size_t n, typename Ring<C>::W *dst, Form f) {
    if (!n) return LF_OK;
    u64 *tmp;
    RET(c->tbuf("stage_aos", n * Ring<C>::RE, &tmp));
    HIPCHK(hipMemcpyAsync(tmp, host, n * Ring<C>::RE * 8, hipMemcpyHostToDevice, c->stream()));
    const auto Ti = Ring<C>::xb_mat(c->xb_Ti);
    launch_aos_to_soa(tmp, dst, n, c->stream(), nullptr, xb_converts(c, f) ? &Ti : nullptr);
    return LF_OK;
}
template <class C>
int down_ring(C *c, const typename Ring<C>::W *src, size_t n, u64 *host, Form f) {
    if (!n) return LF_OK;
    u64 *tmp;
    RET(c->tbuf("stage_aos", n * Ring<C>::RE, &tmp));
    const auto T = Ring<C>::xb_mat(c->xb_T);
    launch_soa_to_aos(src, tmp, n, c->stream(), nullptr, xb_converts(c, f) ? &T : nullptr);
    HIPCHK(hipMemcpyAsync(host, tmp, n * Ring<C>::RE * 8, hipMemcpyDeviceToHost, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));
    return LF_OK;
}

// ---- where the O(n) array arguments of an entry point live --------------------------------------------------------------------------------------------
// Origin::host (every lf_* call without the suffix): pageable host memory, staged through `stage_aos` as above.  Origin::device (the _dev twins): the caller's own
// memory on the context's device, same AoS layout; the relayout kernels read and write it in place, nothing is staged.  What the host cannot see it lets the
// device check: the checked relayout raises a flag word on an input word >= p, the flag comes back in front of a synchronise the call performs anyway, results go
// into the caller's buffer only while the flag is down (launch_soa_to_aos's unless_flag), and the call returns LF_ERR_INVALID.  A body with several input
// tables (mle_eval_batch, lincomb, horner_combine, the sumcheck begins) relayouts each into the scratch of the host path and acts on the flag once, at the end;
// one with several result tables (decompose, layout 1) stores each behind the flag (store_ring) and ends in DevIo::finish.
// (Origin and the check itself: lf_dev_ptr.h, which the LatticeFold+ slice includes as well)
using lfdev::Origin;
using lfdev::range_inside;
// THE pointer check of every _dev entry point, before anything is enqueued: device memory of `device`, 8-byte aligned, `bytes` bytes inside one allocation.
// A host or pinned pointer, managed memory, another device's memory, a range that runs off its allocation: LF_ERR_INVALID, never a launch
using lfdev::dev_array_check;
static_assert(LF_OK == 0 && LF_ERR_INVALID == -1, "dev_array_check returns 0 / -1");
template <class C>
struct DevIo {
    C *c;
    const bool dev;
    u32 *flag = nullptr, *hflag = nullptr;   // device word / its pinned copy; null: nothing of this call is checked on the device (host origin, or no array input)
    DevIo(C *c_, Origin o) : c(c_), dev(o == Origin::device) {}
    // an array argument of n ring elements (after the call's state and length checks, before anything is enqueued)
    int array(const void *p, size_t n) const { return dev && n ? dev_array_check(c->device, p, n * Ring<C>::RE * 8) : LF_OK; }
    // the call has device inputs: lower the flag, in stream
    int begin() {
        if (!dev) return LF_OK;
        RET(c->dev_flag(&flag, &hflag));
        *hflag = 0;
        HIPCHK(hipMemsetAsync(flag, 0, 4, c->stream()));
        return LF_OK;
    }
    // enqueue the flag's way home; bad() is valid after the next synchronise of the stream
    int fetch() {
        if (flag) HIPCHK(hipMemcpyAsync(hflag, flag, 4, hipMemcpyDeviceToHost, c->stream()));
        return LF_OK;
    }
    bool bad() const { return flag && *(volatile u32 *)hflag != 0; }
    // an input array and `out` of a call whose sizes differ (na, nb ring elements): any overlap is refused, an in-place form has no meaning
    int disjoint(const void *a, size_t na, const void *b, size_t nb) const {
        const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
        return !dev || pa + na * Ring<C>::RE * 8 <= pb || pb + nb * Ring<C>::RE * 8 <= pa ? LF_OK : LF_ERR_INVALID;
    }
    // the same for an array that is not made of ring elements (the eq table of lf_build_eq_dev)
    int words(const void *p, size_t n) const { return dev && n ? dev_array_check(c->device, p, n * 8) : LF_OK; }
    // the flag word itself: bit 0 a word >= p, bit 1 an eq table that is not slot-constant (launch_slot_const_check)
    u32 raised() const { return flag ? *(volatile u32 *)hflag : 0; }
    // the end of a device-origin call whose results are stored already, or that has none: the flag comes home, the stream is synchronised
    int finish() {
        RET(fetch());
        HIPCHK(hipStreamSynchronize(c->stream()));
        return bad() ? LF_ERR_INVALID : LF_OK;
    }
};
template <class C>
int up_ring(DevIo<C> &io, const u64 *src, size_t n, typename Ring<C>::W *dst, Form f) {
    if (!io.dev) return up_ring(io.c, src, n, dst, f);
    const auto Ti = Ring<C>::xb_mat(io.c->xb_Ti);
    launch_aos_to_soa(src, dst, n, io.c->stream(), io.flag, xb_converts(io.c, f) ? &Ti : nullptr);   // (the caller's words are tested, then converted)
    return LF_OK;
}
// the result of a call, complete on return; from device inputs that were not canonical: LF_ERR_INVALID and `out` untouched
template <class C>
int down_ring(DevIo<C> &io, const typename Ring<C>::W *src, size_t n, u64 *out, Form f) {
    if (!io.dev) return down_ring(io.c, src, n, out, f);
    const auto T = Ring<C>::xb_mat(io.c->xb_T);
    launch_soa_to_aos(src, out, n, io.c->stream(), io.flag, xb_converts(io.c, f) ? &T : nullptr);
    return io.finish();
}
// one of several result tables of a device-origin call: stored while the flag is down, no synchronise -- io.finish() ends the call
template <class C>
void store_ring(DevIo<C> &io, const typename Ring<C>::W *src, size_t n, u64 *out, Form f) {
    const auto T = Ring<C>::xb_mat(io.c->xb_T);
    launch_soa_to_aos(src, out, n, io.c->stream(), io.flag, xb_converts(io.c, f) ? &T : nullptr);
}
template <class C, class T>
int upload_consts(C *c, const std::string &name, const std::vector<T> &v, T **out) {
    RET(c->tbuf(name, v.size() + 8, out));
    return Ring<C>::h2d_consts(c, *out, v.data(), v.size() * sizeof(T));
}

// a launcher's negative result (lf_i8_launch.h) as an ABI code: a shape nothing handles / a failed HIP call
inline int i8_rc(int r) { return r == i8mma::I8_ERR_HIP ? LF_ERR_HIP : LF_ERR_UNSUPPORTED; }

// ---- general commit, host side -----------------------------------------------------------------------------------------------------------------------
// The contraction of `batch` operands whose digit words [NP][RE][ntiles] of this rank's columns the caller's pass cut(b, pre, ntiles) writes: NP = 10 (5 on
// BabyBear) for an arbitrary element, 5 for the int32 planes of a witness handle, fewer for the digits of a gadget decomposition (ajtai_i8g_planes_base).
// out_dev: canonical u64 [batch][kappa][RE] NTT form, AoS (PARTIAL when sharded).
template <class C, class Cut>
int commit_dev_pre(C *c, u32 NP, u32 batch, u64 *out_dev, bool timed, Cut &&cut) {
    typedef Ring<C> R;
    typedef typename R::W W;
    if (!c->A_loaded || !c->i8_nch || !c->dAb) return LF_ERR_STATE;
    const AjtaiI8Ring I = R::i8();
    const u32 nch = c->i8_nch, kc = c->i8_kc, MT = ajtai_i8_row_tiles(I, kc);
    const size_t ntiles = (c->nA + 7) / 8, chunk_bytes = ntiles * (I.RD / 8) * MT * 1024;
    const u32 nwg = c->tn.i8g_wgs > 0 ? (u32)c->tn.i8g_wgs : 256;   // (default: one per CU)
    size_t pw, dw, sw;
    if (ajtai_i8g_scratch(I, MT, c->nA, NP, nwg, &pw, &dw, &sw) != 0) return LF_ERR_UNSUPPORTED;
    unsigned long long *pre;
    int32_t *part, *dsum;
    long long *sum;
    u64 *co;
    W *cf, *ntt;
    RET(c->tbuf("i8g_pre", (size_t)NP * R::RE * ntiles, &pre));
    RET(c->tbuf("i8g_part", pw, &part));
    RET(c->tbuf("i8g_dsum", dw, &dsum));
    RET(c->tbuf("i8g_sum", sw, &sum));
    RET(c->tbuf(R::i8g_co, (size_t)R::RE * c->kappa, &co));
    if constexpr (R::montgomery) RET(c->tbuf("i8g_cf", (size_t)R::RE * c->kappa, &cf));
    else cf = co;   // the kernel's canonical coefficient planes ARE the device form
    RET(c->tbuf("i8g_ntt", (size_t)R::RE * c->kappa, &ntt));
    for (u32 b = 0; b < batch; b++) {
        const size_t ev = timed ? c->ev_begin(1) : 0;   // the whole device side of one commitment: digit pass, contraction, recombination, CRT
        cut(b, pre, ntiles);
        for (u32 ch = 0; ch < nch; ch++) {
            const u32 row0 = ch * kc, kn = c->kappa - row0 < kc ? c->kappa - row0 : kc;
            const int g = launch_ajtai_i8g(I, c->dAb + (size_t)ch * chunk_bytes, MT, pre, ntiles, c->nA, kn, row0, c->kappa, NP, nwg, part, dsum, sum, co, c->stream(), 0,
                                           c->tn.i8g_prof);
            if (g < 0) return i8_rc(g);
        }
        if constexpr (R::montgomery) launch_aos_to_soa(co, cf, c->kappa, c->stream());   // BabyBear only: the kernel's element-major canonical words -> Montgomery planes
        launch_crt_fwd(R::tab(c), cf, ntt, c->kappa, c->stream());
        launch_soa_to_aos(ntt, out_dev + (size_t)b * c->kappa * R::RE, c->kappa, c->stream());
        if (timed) c->ev_end(ev);
    }
    return LF_OK;
}
// General commitments from the resident byte planes of A (lf_ajtai_i8g.hip): AjtaiCommitmentScheme::commit_ntt (commitment_scheme.rs:37-54,75-77) for
// `batch` vectors F [batch][RE][ldF] in NTT form (pointing at this rank's first column), or Witness::commit (arith.rs:357-362) for the centred int32
// coefficient planes of a witness handle (F null, batch 1): five balanced base-128 digit planes, no NTT of the witness.
template <class C>
int commit_dev_i8g(C *c, const typename Ring<C>::W *F, size_t ldF, u32 batch, const int32_t *planes, size_t ldp, u64 *out_dev, bool timed) {
    typedef Ring<C> R;
    const u32 NP = planes ? ajtai_i8g_planes_i32() : ajtai_i8g_planes_general(R::i8());
    return commit_dev_pre(c, NP, batch, out_dev, timed, [&](u32 b, unsigned long long *pre, size_t ntiles) {
        if (planes) launch_i8g_cut_i32(planes, ldp, c->nA, R::RE, NP, pre, ntiles, c->stream());
        else launch_i8g_cut_ntt(c->d_icrt, c->d_icrt_sp_val, c->d_icrt_sp_col, F + (size_t)b * R::RE * ldF, ldF, c->nA, NP, pre, ntiles, c->stream());
    });
}
// Witness::commit into device memory (kappa ring elements, canonical AoS; unsharded contexts)
template <class C>
int witness_commit_dev(C *c, const lf_witness *w, u64 *out_dev) { return commit_dev_i8g(c, nullptr, 0, 1, w->planes + c->A_col0, w->N, out_dev, false); }

// The commitments of a fold step: digit planes k0 .. k0+NP-1 of `planes` (this rank's column slice) -> out_dev canonical u64 [NP][kappa][RE], NTT form, AoS
// (PARTIAL when sharded).  wit (optional): the witness `planes` belong to (R::bit_planes).  Buffer names and sizes are what they were per ring: a step's
// memory footprint depends on them.
template <class C>
int commit_planes_i8(C *c, const int32_t *planes, size_t ld, u32 k0, u32 NP, u64 *out_dev, const lf_witness *wit = nullptr) {
    typedef Ring<C> R;
    typedef typename R::W W;
    constexpr size_t RE = R::RE;
    const AjtaiI8Ring I = R::i8();
    const u32 nch = c->i8_nch, kc = c->i8_kc, MT = ajtai_i8_row_tiles(I, kc), maxp = ajtai_i8_max_planes_mt(I, MT);
    const size_t ntiles = (c->nA + 7) / 8, chunk_bytes = ntiles * (I.RD / 8) * MT * 1024;
    // One persistent workgroup per CU fills its LDS (157 KB): on a fully occupied chip the latency-bound round kernels of the other lane
    // cannot be placed until a commit workgroup retires.  7/8 of the CUs (28 of 32 per XCD) leaves them room: C4 26.1 -> 25.0 ms/step
    // (measured 256 / 240 / 224 / 192 / 160 / 128 workgroups: 26.1 / 26.3 / 25.0 / 25.1 / 26.1 / 28.2 ms).
    u32 nwg = c->tn.i8_wgs > 0 ? (u32)c->tn.i8_wgs : 224;
    if (nwg > ntiles) nwg = (u32)ntiles;
    const u32 nslots = nwg < 16 ? 16 : nwg;    // (two plane groups run as 2 x 8 chunks at least: launch_ajtai_i8)
    int32_t *part, *dsum;
    long long *sum;
    u64 *coef;
    W *cf = nullptr, *ntt;
    const u32 NTmax = ajtai_i8_col_tiles(I, maxp);
    RET(c->tbuf("i8_part", ajtai_i8_part_words(nslots, MT, NTmax), &part));
    RET(c->tbuf("i8_dsum", (size_t)nslots * maxp * I.RD, &dsum));
    RET(c->tbuf("i8_sum", ajtai_i8_sum_words(I, MT, NTmax, maxp), &sum));
    RET(c->tbuf("i8_coef", RE * NP * c->kappa, &coef));
    if constexpr (R::montgomery) RET(c->tbuf("i8_cf", RE * NP * c->kappa, &cf));
    RET(c->tbuf("i8_ntt", RE * NP * c->kappa, &ntt));
    const u32 *bits;
    RET(R::bit_planes(c, planes, wit, &bits));
    const size_t bits_nw = (c->N + 511) / 512 * 16;          // words per row of the bit-plane form (positions padded to 512)
    const u32 bits_rows = 16 * ((c->P.K + 15) / 16) + 1;
    for (u32 p0 = 0; p0 < NP; p0 += maxp) {
        const u32 np = NP - p0 < maxp ? NP - p0 : maxp;
        u64 *co = coef + RE * p0 * c->kappa;   // block of this plane group: coefficient planes [RE][np*kappa] (Goldilocks), element-major [np*kappa][RE] (BabyBear)
        for (u32 ch = 0; ch < nch; ch++) {
            const u32 row0 = ch * kc, kn = c->kappa - row0 < kc ? c->kappa - row0 : kc;
            size_t ev = c->ev_begin(1);
            int g = launch_ajtai_i8(I, c->dAb + (size_t)ch * chunk_bytes, MT, planes, ld, c->nA, kn, row0, c->kappa, k0 + p0, np, nwg, part, dsum, sum, co, c->stream(),
                                    c->tn.i8_couple_w, c->tn.i8_prof, bits, bits_nw, bits_rows);
            c->ev_end(ev);
            if (g < 0) return i8_rc(g);
        }
        const size_t ne = (size_t)np * c->kappa;
        const W *src;
        if constexpr (R::montgomery) { launch_aos_to_soa(co, cf, ne, c->stream()); src = cf; }   // canonical -> Montgomery planes
        else src = co;                                                                         // the kernel's canonical planes ARE the device form
        launch_crt_fwd(R::tab(c), src, ntt, ne, c->stream());
        launch_soa_to_aos(ntt, out_dev + (size_t)p0 * c->kappa * RE, ne, c->stream());
    }
    return LF_OK;
}

inline bool pow2(u64 b) { return b >= 2 && (b & (b - 1)) == 0; }

// ---- the entry points: everything after the argument checks, the external-basis wrapper and the ring dispatch ----------------------------------------
template <class R>
struct ring_ops;
template <class C>
struct ring_ops<Ring<C>> {
    typedef Ring<C> R;
    typedef typename R::W W;
    typedef typename R::Ext Ext;
    typedef typename R::ExtC ExtC;
    typedef typename R::Part Part;
    static constexpr size_t RE = R::RE, TAU = R::TAU;

    // ---- set-up ----
    // install_tables after the ring's own table build: the dense inverse CRT map icrt [RE][RE] (canonical) and its rows in compressed form for the digit pass
    // of the general commitment (k_i8g_cut_ntt): the shipped tables have one entry per slot
    static int install_icrt(C *c, const u64 *icrt) {
        std::vector<W> mat(RE * RE), sv(RE * 8, 0);
        std::vector<u32> sc(RE * 8, 0xFFFFFFFFu);
        for (size_t i = 0; i < RE * RE; i++) mat[i] = R::from_canon(icrt[i]);
        if (!c->d_icrt) HIPCHK(lf_dev_malloc(&c->d_icrt, mat.size() * sizeof(W)));
        HIPCHK(hipMemcpy(c->d_icrt, mat.data(), mat.size() * sizeof(W), hipMemcpyHostToDevice));
        bool sparse = true;
        for (size_t r = 0; r < RE && sparse; r++) {
            int q = 0;
            for (size_t col = 0; col < RE; col++)
                if (icrt[r * RE + col]) {
                    if (q == 8) { sparse = false; break; }
                    sv[r * 8 + q] = mat[r * RE + col]; sc[r * 8 + q] = (u32)col; q++;
                }
        }
        if (sparse) {
            if (!c->d_icrt_sp_val) { HIPCHK(lf_dev_malloc(&c->d_icrt_sp_val, sv.size() * sizeof(W))); HIPCHK(lf_dev_malloc(&c->d_icrt_sp_col, sc.size() * sizeof(u32))); }
            HIPCHK(hipMemcpy(c->d_icrt_sp_val, sv.data(), sv.size() * sizeof(W), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(c->d_icrt_sp_col, sc.data(), sc.size() * sizeof(u32), hipMemcpyHostToDevice));
        } else if (c->d_icrt_sp_val) {
            (void)hipFree(c->d_icrt_sp_val); (void)hipFree(c->d_icrt_sp_col);
            c->d_icrt_sp_val = nullptr; c->d_icrt_sp_col = nullptr;
        }
        return LF_OK;
    }
    // A lives on the device in ONE form: coefficient form, cut into bytes, in MFMA operand order (lf_ajtai_i8.hip) -- what the digit-plane commitments of a fold
    // step and the general commitments (lf_ajtai_i8g.hip) both stream.  Built once per matrix, one row at a time through one row buffer (uploaded, or filled from
    // the seed), so the peak is the byte planes plus one row.  The context holds NO matrix from the first line that can fail to the last: kappa, the column
    // slice, the chunking and "A is resident" are published together, on success only.
    static int ajtai_install(C *c, size_t kappa, size_t n, const u64 *A_host, u64 seed) {
        if (kappa > R::max_kappa) return LF_ERR_INVALID;
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        size_t col0, cnt;
        RET(c->shard_columns(n, &col0, &cnt));   // a sharded rank keeps only its column slice of the caller's matrix
        c->drop_matrix();
        const AjtaiI8Ring I = R::i8();
        const u32 maxr = ajtai_i8_max_rows(I), nch = ((u32)kappa + maxr - 1) / maxr, kc = ((u32)kappa + nch - 1) / nch, MT = ajtai_i8_row_tiles(I, kc);
        const size_t chunk_bytes = (cnt + 7) / 8 * (I.RD / 8) * MT * 1024, bytes = chunk_bytes * nch + ajtai_i8_slack_bytes();
        unsigned char *Ab = nullptr;
        HIPCHK(lf_dev_malloc(&Ab, bytes));
        const int rc = [&]() -> int {
            HIPCHK(hipMemsetAsync(Ab, 0, bytes, c->stream()));
            W *row;
            RET(c->tbuf("i8_prep_row", RE * cnt, &row));
            for (size_t i = 0; i < kappa; i++) {
                if (A_host) RET(up_ring(c, A_host + (i * n + col0) * RE, cnt, row, Form::ntt));
                else launch_fill_ajtai(row, 1, cnt, n, col0, seed, c->stream(), (u32)i);
                RET(R::pack_row(c, row, cnt, (u32)i % kc, MT, Ab + (i / kc) * chunk_bytes));
            }
            HIPCHK(hipStreamSynchronize(c->stream()));
            return LF_OK;
        }();
        if (rc != LF_OK) (void)hipStreamSynchronize(c->stream());   // nothing enqueued above still uses the scratch or Ab when they go
        for (const char *name : {"i8_prep_row", "i8_prep_coef", "i8_prep_canon", "stage_aos"}) c->drop_buf(name);
        if (rc != LF_OK) { (void)hipFree(Ab); return rc; }
        c->dAb = Ab;
        c->kappa = (u32)kappa;
        c->nA = cnt; c->nA_total = n; c->A_col0 = col0;
        c->i8_nch = nch; c->i8_kc = kc;
        c->A_loaded = true;
        return LF_OK;
    }
    // lf_ccs_load after the ring's envelope check (limits on s, t, q, K, L, d, b, B: per ring): the checks that need no context, then the descriptor, the CSR
    // arrays and their CSC form on the device
    static int ccs_load(C *c, const lf_params *P, const u32 *const *rowptr, const u32 *const *col, const u64 *const *val, const u32 *S_off, const u32 *S_idx,
                        const u64 *cc) {
        const size_t m = (size_t)1 << P->s, N = (size_t)P->wit_len * P->L, n = (size_t)P->l + 1 + P->wit_len;
        if (N > m) return LF_ERR_SIZE_BOUNDS;  // sanity_check, nifs.rs:165-173
        {   // the reference indexes comb values by matrix index: multisets must concatenate to 0..t-1
            u32 next = 0;
            for (u32 i = 0; i < P->q; i++)
                for (u32 k = S_off[i]; k < S_off[i + 1]; k++)
                    if (S_idx[k] != next++) return LF_ERR_UNSUPPORTED;
            if (next != P->t || S_off[P->q] > 16) return LF_ERR_UNSUPPORTED;
        }
        RET(lf_validate_csr(P->t, m, n, rowptr, col, val, RE, R::modulus));   // before any context state is touched
        for (size_t k = 0; k < (size_t)P->q * RE; k++)
            if (cc[k] >= R::modulus) return LF_ERR_INVALID;
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        c->free_ccs();
        c->P = *P; c->N = N; c->m = m; c->n = n;
        memset(&c->desc, 0, sizeof(c->desc));
        c->desc.t = P->t; c->desc.q = P->q;
        for (u32 i = 0; i <= P->q; i++) c->desc.S_off[i] = S_off[i];
        for (u32 k = 0; k < S_off[P->q]; k++) c->desc.S_idx[k] = S_idx[k];
        if constexpr (R::general_csr)
            for (u32 i = 0; i < P->q; i++)
                for (u32 k = S_off[i]; k < S_off[i + 1]; k++) { c->desc.ms[k] = i; c->desc.first[k] = (k == S_off[i]); }
        u64 one[RE], mone[RE];
        R::ring_from_u64(1, one);
        R::ring_from_u64(R::modulus - 1, mone);
        for (u32 i = 0; i < P->q; i++) {
            const u64 *ci = cc + (size_t)i * RE;
            for (size_t w = 0; w < RE; w++) c->desc.c[i][w] = R::from_canon(ci[w]);
            c->desc.c_unit[i] = !memcmp(ci, one, sizeof(one)) ? 1 : (!memcmp(ci, mone, sizeof(mone)) ? -1 : 0);
        }
        // every device array is registered in the context as soon as it exists, so a failure half-way leaks nothing (free_ccs frees them)
        auto dalloc = [](auto &vec, size_t bytes) -> void * {
            void *ptr = nullptr;
            if (lf_dev_malloc(&ptr, bytes) != hipSuccess) return nullptr;
            vec.push_back((typename std::remove_reference<decltype(vec)>::type::value_type)ptr);
            return ptr;
        };
        for (u32 j = 0; j < P->t; j++) {
            const size_t nnz = rowptr[j][m];
            std::vector<W> conv;
            const W *v;
            if constexpr (R::montgomery) {
                conv.resize(nnz * RE + 1);
                for (size_t k = 0; k < nnz * RE; k++) conv[k] = R::from_canon(val[j][k]);
                v = conv.data();
            } else v = val[j];   // canonical words are the device form
            std::vector<u32> cp(n + 1, 0), ri(nnz + 1);
            std::vector<W> vT(nnz * RE + 1);
            for (size_t k = 0; k < nnz; k++) cp[col[j][k] + 1]++;
            for (size_t i = 0; i < n; i++) cp[i + 1] += cp[i];
            std::vector<u32> fill(cp.begin(), cp.end() - 1);
            for (size_t r = 0; r < m; r++)
                for (u32 k = rowptr[j][r]; k < rowptr[j][r + 1]; k++) {
                    const u32 pos = fill[col[j][k]]++;
                    ri[pos] = (u32)r;
                    memcpy(&vT[(size_t)pos * RE], v + (size_t)k * RE, RE * sizeof(W));
                }
            void *drp = dalloc(c->d_rowptr, (m + 1) * 4), *dci = dalloc(c->d_col, (nnz + 1) * 4), *dv = dalloc(c->d_val, (nnz + 1) * RE * sizeof(W));
            void *dcp = dalloc(c->d_colptr, (n + 1) * 4), *dri = dalloc(c->d_rowidx, (nnz + 1) * 4), *dvT = dalloc(c->d_valT, (nnz + 1) * RE * sizeof(W));
            if (!drp || !dci || !dv || !dcp || !dri || !dvT) return LF_ERR_HIP;
            HIPCHK(hipMemcpy(drp, rowptr[j], (m + 1) * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dci, col[j], nnz * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dv, v, nnz * RE * sizeof(W), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dcp, cp.data(), (n + 1) * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dri, ri.data(), nnz * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dvT, vT.data(), nnz * RE * sizeof(W), hipMemcpyHostToDevice));
            std::vector<u32> plan;   // lf_spmv_t: the heavy columns of M_j as work items (lf_spmv_t_plan.h)
            u32 nitems, ncols;
            c->spmvt_min = c->spmvt_min_next;
            lfk::spmv_t_plan(n, cp.data(), c->spmvt_min, &plan, &nitems, &ncols);
            c->d_spmvt_plan.push_back(nullptr);
            c->spmvt_items.push_back(nitems); c->spmvt_cols.push_back(ncols);
            if (nitems) {
                HIPCHK(lf_dev_malloc(&c->d_spmvt_plan.back(), plan.size() * 4));
                HIPCHK(hipMemcpy(c->d_spmvt_plan.back(), plan.data(), plan.size() * 4, hipMemcpyHostToDevice));
            }
        }
        if constexpr (R::general_csr) {
            const size_t rows_used = n < m ? n : m;
            c->ccs_general = false;
            for (u32 jj = 0; jj < P->t; jj++)
                if ((size_t)rowptr[jj][m] * 2 > rows_used * 3) c->ccs_general = true;
            c->shc_r0 = (size_t)-1;
            c->live_rows = lflive::live_rows(P->t, m, rowptr);   // the trailing empty rows are skipped by M z, the linearization rounds and G (lf_live_rows.h)
        }
        c->have_ccs = true;
        return LF_OK;
    }

    // ---- a5: general commitments through the ABI ----
    // Both re-read the environment switches, as every prover entry point does (the BabyBear bodies did not before they were merged: nothing in the general
    // commit path of that ring consumes a tunable, so the read changes nothing there until the next linearize / fold step reads them again anyway).
    static int ajtai_commit(C *c, const u64 *f, size_t n, size_t batch, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->A_loaded) return LF_ERR_STATE;
        if (n != c->nA_total) return LF_ERR_INVALID;  // CommitmentError::WrongWitnessLength(n, width)
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(f, batch * n));
        W *F;
        u64 *o;
        RET(c->tbuf("io_a", batch * n * RE, &F));
        RET(c->tbuf(R::io_out, batch * c->kappa * RE, &o));
        RET(io.begin());
        for (size_t b = 0; b < batch; b++) RET(up_ring(io, f + b * n * RE, n, F + b * RE * n, Form::ntt));
        c->tn = Tunables::read(R::lut_min_default);
        c->ev_reset();
        RET(commit_dev_i8g(c, F + c->A_col0, n, (u32)batch, nullptr, 0, o, true));   // timed: lf_last_kernel_stats reports the stand-alone kernel
        RET(io.fetch());
        c->ev_collect();   // (synchronises the lanes)
        if (io.bad()) return LF_ERR_INVALID;
        return R::commit_finish(c, o, batch * c->kappa * RE, out);
    }
    // commit_coeff / decompose_and_commit_{coeff,ntt} (commitment_scheme.rs:81-113): element i of f [batch][count] (coefficient form, or NTT form: ntt_in)
    // becomes columns [i L, (i + 1) L) of the committed vector, its balanced base-2^lb digits (lb 0, L 1: the element itself).  The count x L vector is never
    // built: the gadget digit pass (lf_i8g_dec.cuh) writes the commit kernel's operand words from the coefficient table, as few planes as the base needs.
    // NTT-form input is inverse-CRT-ed into one coefficient table first (one pass over count elements; the fused form of k_i8g_cut_ntt would map 32 elements
    // = 32 L columns per block -- DESIGN.md, k_ajtai_i8g row).
    static int ajtai_commit_gadget(C *c, const u64 *f, bool ntt_in, size_t count, u32 lb, u32 L, size_t batch, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->A_loaded) return LF_ERR_STATE;
        if (count > c->nA_total || count * L != c->nA_total) return LF_ERR_INVALID;   // CommitmentError::WrongWitnessLength
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(f, batch * count));
        W *F, *X = nullptr;
        u64 *o;
        RET(c->tbuf("io_a", batch * count * RE, &F));
        if (ntt_in) RET(c->tbuf("io_c", count * RE, &X));
        RET(c->tbuf(R::io_out, batch * c->kappa * RE, &o));
        RET(io.begin());
        for (size_t b = 0; b < batch; b++) RET(up_ring(io, f + b * count * RE, count, F + b * RE * count, ntt_in ? Form::ntt : Form::coeff));
        c->tn = Tunables::read(R::lut_min_default);
        c->ev_reset();
        const u32 NP = lb ? ajtai_i8g_planes_base(R::i8(), 1ull << lb) : ajtai_i8g_planes_general(R::i8());
        RET(commit_dev_pre(c, NP, (u32)batch, o, true, [&](u32 b, unsigned long long *pre, size_t ntiles) {   // timed: the ICRT, digit pass and contraction
            const W *src = F + (size_t)b * RE * count;
            if (ntt_in) { launch_icrt_dense(c->d_icrt, src, X, count, c->stream()); src = X; }
            launch_i8g_cut_dec(src, count, c->A_col0, c->nA, L, lb, c->digit_mode, NP, pre, ntiles, c->stream());
        }));
        RET(io.fetch());
        c->ev_collect();   // (synchronises the lanes)
        if (io.bad()) return LF_ERR_INVALID;
        return R::commit_finish(c, o, batch * c->kappa * RE, out);
    }

    // ---- a1/a2/a3 ----
    static int ntt_fwd(C *c, const u64 *in, u64 *out, size_t count, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(in, count));
        RET(io.array(out, count));
        W *a, *b;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * RE, &b));
        RET(io.begin());
        RET(up_ring(io, in, count, a, Form::coeff));
        launch_crt_fwd(R::tab(c), a, b, count, c->stream());
        return down_ring(io, b, count, out, Form::ntt);
    }
    static int ntt_inv(C *c, const u64 *in, u64 *out, size_t count, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(in, count));
        RET(io.array(out, count));
        W *a, *b;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * RE, &b));
        RET(io.begin());
        RET(up_ring(io, in, count, a, Form::ntt));
        launch_icrt_dense(c->d_icrt, a, b, count, c->stream());
        return down_ring(io, b, count, out, Form::coeff);
    }
    // lf_ring_mul: out[x] = sum_{i < n_terms} a_i[x] * b_i[x], all three arrays in the same form.  NTT form: the slot-wise product, in an external basis between
    // the basis-changing relayouts like every NTT-form array; coefficient form: transforms and product in one kernel, nothing converted.  `out` may BE table 0
    // of a or of b when there is one term (the result is complete in a scratch table before `out` is written); any other overlap of a device `out` is refused
    static int ring_mul(C *c, const u64 *a, const u64 *b, size_t n_terms, size_t count, int form, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        const Form f = form == LF_FORM_COEFF ? Form::coeff : Form::ntt;
        DevIo<C> io(c, org);
        RET(io.array(a, n_terms * count));
        RET(io.array(b, n_terms * count));
        RET(io.array(out, count));
        for (const u64 *in : {a, b})
            if (n_terms != 1 || in != out) RET(io.disjoint(in, n_terms * count, out, count));
        W *o;
        RET(c->tbuf("io_b", count * RE, &o));
        RET(io.begin());
        if (f == Form::ntt) {   // the kernel reads the AoS operands themselves (the caller's device arrays, or their staged copies) and relayouts them in LDS
            const u64 *da = a, *db = b;
            if (!io.dev) {
                u64 *sa, *sb;
                RET(c->tbuf("io_a", n_terms * count * RE, &sa));
                RET(c->tbuf("io_c", n_terms * count * RE, &sb));
                if (count) {
                    HIPCHK(hipMemcpyAsync(sa, a, n_terms * count * RE * 8, hipMemcpyHostToDevice, c->stream()));
                    HIPCHK(hipMemcpyAsync(sb, b, n_terms * count * RE * 8, hipMemcpyHostToDevice, c->stream()));
                }
                da = sa; db = sb;
            }
            const auto Ti = R::xb_mat(c->xb_Ti);
            launch_ring_mul_ntt(R::tab(c), da, db, n_terms, count, o, c->stream(), io.flag, xb_converts(c, f) ? &Ti : nullptr);
        } else {
            W *A, *B;
            RET(c->tbuf("io_a", n_terms * count * RE, &A));
            RET(c->tbuf("io_c", n_terms * count * RE, &B));
            for (size_t i = 0; i < n_terms; i++) {
                RET(up_ring(io, a + i * count * RE, count, A + i * RE * count, f));
                RET(up_ring(io, b + i * count * RE, count, B + i * RE * count, f));
            }
            launch_ring_mul_coeff(R::tab(c), c->d_icrt, A, B, n_terms, count, o, c->stream());
        }
        return down_ring(io, o, count, out, f);
    }
    static int decompose(C *c, const u64 *in, size_t count, u64 base, unsigned digits, int layout, u64 *out, Origin org = Origin::host) {
        if (!pow2(base)) return LF_ERR_UNSUPPORTED;
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(in, count));
        RET(io.array(out, count * digits));
        RET(io.disjoint(in, count, out, count * digits));
        W *a, *b;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * digits * RE, &b));
        RET(io.begin());
        RET(up_ring(io, in, count, a, Form::coeff));
        launch_decompose(a, count, base, digits, layout, b, c->stream(), c->digit_mode);
        if (layout == 0) return down_ring(io, b, count * digits, out, Form::coeff);
        if (io.dev) {   // every digit table is stored behind the flag: input that was not canonical leaves none of them written
            for (unsigned k = 0; k < digits; k++) store_ring(io, b + (size_t)k * RE * count, count, out + (size_t)k * count * RE, Form::coeff);
            return io.finish();
        }
        for (unsigned k = 0; k < digits; k++) RET(down_ring(c, b + (size_t)k * RE * count, count, out + (size_t)k * count * RE, Form::coeff));
        return LF_OK;
    }
    static int recompose(C *c, const u64 *in, size_t count_out, u64 base, unsigned digits, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(in, count_out * digits));
        RET(io.array(out, count_out));
        RET(io.disjoint(in, count_out * digits, out, count_out));
        W *a, *b;
        RET(c->tbuf("io_a", count_out * digits * RE, &a));
        RET(c->tbuf("io_b", count_out * RE, &b));
        RET(io.begin());
        RET(up_ring(io, in, count_out * digits, a, Form::coeff));
        launch_recompose(a, count_out, base, digits, b, c->stream());
        return down_ring(io, b, count_out, out, Form::coeff);
    }
    static int linf_check(C *c, const u64 *f_ntt, size_t count, u64 bound, int unsigned_variant, int *ok, u64 *max_out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(f_ntt, count));
        W *a, *b;
        u64 *mx;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * RE, &b));
        RET(c->tbuf("small_dev", 4096, &mx));
        RET(io.begin());
        RET(up_ring(io, f_ntt, count, a, Form::ntt));
        launch_icrt_dense(c->d_icrt, a, b, count, c->stream());
        u64 m = 0;
        RET(io.fetch());   // (in front of the synchronise of either download)
        if (unsigned_variant) {
            // literal Witness::within_bound (arith.rs:372-386): canonical coefficient < bound.  The maximum is taken over CANONICAL words, so the table comes
            // down through down_ring (BabyBear planes hold Montgomery words); a maximum does not depend on the layout
            std::vector<u64> h(count * RE);
            RET(down_ring(c, b, count, h.data(), Form::coeff));
            for (u64 v : h) m = v > m ? v : m;
        } else {
            launch_linf(b, count, mx, c->stream());
            RET(down_small(c, mx, 1, &m));
        }
        if (io.bad()) return LF_ERR_INVALID;
        if (max_out) *max_out = m;
        *ok = m < bound;
        return LF_OK;
    }

    // ---- a8/a9/a11 ----
    static std::vector<Ext> load_point(const u64 *point, unsigned nv) {
        std::vector<Ext> pt(nv);
        for (unsigned i = 0; i < nv; i++) pt[i] = R::ext_load(point + TAU * i);
        return pt;
    }
    static int build_eq(C *c, const u64 *point, unsigned nv, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        const size_t n = (size_t)1 << nv;
        DevIo<C> io(c, org);
        RET(io.words(out, TAU * n));
        W *eq;
        RET(c->tbuf("io_a", TAU * n, &eq));
        RET(build_eq_dev(c, load_point(point, nv).data(), nv, eq));
        if (io.dev) {   // the transposition below as a kernel into the caller's buffer; in an external basis the entries leave converted, as the host twin's do
            const auto T = R::xb_mat(c->xb_T);
            launch_ext_to_aos(eq, out, n, c->stream(), xb_converts(c, Form::ntt) ? &T : nullptr);
            return io.finish();
        }
        std::vector<W> h(TAU * n);
        HIPCHK(hipMemcpyAsync(h.data(), eq, h.size() * sizeof(W), hipMemcpyDeviceToHost, c->stream()));
        HIPCHK(hipStreamSynchronize(c->stream()));
        for (size_t i = 0; i < n; i++)
            for (size_t q = 0; q < TAU; q++) out[TAU * i + q] = R::canon(h[q * n + i]);
        return LF_OK;
    }
    static int mle_eval_batch(C *c, const u64 *tables, size_t ntables, size_t len, const u64 *point, unsigned nv, u64 *out, Origin org = Origin::host) {
        const size_t n = (size_t)1 << nv;
        if (len > n || len == 0) return LF_ERR_INVALID;   // MleEvaluationError::IncorrectLength
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(tables, ntables * len));
        W *eq, *X;
        Part *partial;
        u64 *o;
        RET(c->tbuf("io_eq", TAU * n, &eq));
        RET(c->tbuf("io_a", ntables * len * RE, &X));
        RET(c->tbuf("red_partial", R::red_partial(ntables * RE), &partial));
        RET(c->tbuf(R::io_out, ntables * RE, &o));   // (the rings name this buffer differently; kept: buffer names are part of a context's memory footprint)
        RET(io.begin());
        RET(build_eq_dev(c, load_point(point, nv).data(), nv, eq));
        for (size_t a = 0; a < ntables; a++) RET(up_ring(io, tables + a * len * RE, len, X + a * RE * len, Form::ntt));
        launch_dot_eq(R::tab(c), X, len, (u32)ntables, eq, n, len, partial, o, c->stream());
        if (!io.dev) return down_small(c, o, ntables * RE, out);
        std::vector<u64> h(ntables * RE);   // the caller's `out` is written only once the flag has come home clean
        RET(io.fetch());
        RET(down_small(c, o, ntables * RE, h.data()));
        if (io.bad()) return LF_ERR_INVALID;
        memcpy(out, h.data(), h.size() * 8);
        return LF_OK;
    }
    static int spmv(C *c, unsigned j, const u64 *z, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        if (j >= c->P.t) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(z, c->n));
        RET(io.array(out, c->m));
        RET(io.disjoint(z, c->n, out, c->m));
        W *zd, *od;
        RET(c->tbuf("io_a", c->n * RE, &zd));
        RET(c->tbuf("io_b", c->m * RE, &od));
        RET(io.begin());
        RET(up_ring(io, z, c->n, zd, Form::ntt));
        if constexpr (R::general_csr) {   // Goldilocks only: dense rows gather whole elements from an element-major z
            if (c->ccs_general) {
                // a device z is that element-major copy already (as in lf_ccs_check_dev) -- unless it is in an external basis: then it is rebuilt from the converted planes
                // (the checked relayout into zd above still runs then: it is the canonical-word test of z; its planes are not read)
                const bool own = io.dev && !xb_converts(c, Form::ntt);
                W *zaos = (W *)z;   // (canonical words are this ring's device form; read only)
                if (!own) RET(c->tbuf("spmv_zaos", c->n * RE, &zaos));
                launch_spmv_rows(R::tab(c), 1, &c->d_rowptr[j], &c->d_col[j], &c->d_val[j], own ? nullptr : zd, 0, c->n, zaos, od, c->m, 0, c->stream());
                return down_ring(io, od, c->m, out, Form::ntt);
            }
        }
        launch_spmv(R::tab(c), c->d_rowptr[j], c->d_col[j], c->d_val[j], zd, c->n, od, c->m, 0, c->stream());
        return down_ring(io, od, c->m, out, Form::ntt);
    }

    // ---- the sumchecks through the ABI (tests / SURVEY 8b): MLSumcheck::prove_as_subprotocol (utils/sumcheck.rs:53-80) split at the transcript ----
    // tables of the current round: the caller's [..][m] in round 1, halved into the other buffer (leading dimension R::halved_ld) by every later round
    static size_t sc_ld(const C *c, size_t n) { return n == c->m ? c->m : R::halved_ld(n); }
    static int sumcheck_lin_begin(C *c, const u64 *tables, const u64 *eq_point, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        const lf_params &P = c->P;
        const size_t m = c->m;
        DevIo<C> io(c, org);
        RET(io.array(tables, (size_t)P.t * m));
        W *mz, *eqb;
        RET(c->tbuf("sc_tab0", (size_t)P.t * RE * m, &mz));
        RET(c->tbuf("sc_eq0", TAU * m, &eqb));
        RET(io.begin());
        if (io.dev) c->sc_round = -1;   // the tables of a sumcheck in progress go now; a new one is active only once the flag has come home clean
        for (u32 j = 0; j < P.t; j++) RET(up_ring(io, tables + (size_t)j * m * RE, m, mz + (size_t)j * RE * m, Form::ntt));
        RET(build_eq_dev(c, load_point(eq_point, P.s).data(), P.s, eqb));
        if (io.dev) RET(io.finish());
        c->sc_round = 0; c->sc_n = m; c->sc_cur = 0;
        return LF_OK;
    }
    static int sumcheck_lin_round(C *c, const u64 *r_prev, u64 *evals_out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (c->sc_round < 0 || c->sc_round >= (int)c->P.s) return LF_ERR_STATE;  // "Prover is not active"
        if ((c->sc_round == 0) != (r_prev == nullptr)) return LF_ERR_STATE;      // "first round should be prover first" / "verifier message is empty"
        HIPCHK(hipSetDevice(c->device));
        const lf_params &P = c->P;
        const size_t m = c->m;
        W *tab[2], *eq[2];
        Part *partial;
        u64 *od;
        RET(c->tbuf("sc_tab0", (size_t)P.t * RE * m, &tab[0]));
        RET(c->tbuf("sc_tab1", (size_t)P.t * RE * R::halved_ld(m / 2), &tab[1]));
        RET(c->tbuf("sc_eq0", TAU * m, &eq[0]));
        RET(c->tbuf("sc_eq1", TAU * R::halved_ld(m / 2), &eq[1]));
        RET(c->tbuf("round_partial", R::lin_partial_words(m), &partial));
        RET(c->tbuf("round_out", R::lin_out_words, &od));
        if (r_prev) {
            const ExtC r = R::ext_const(c, R::ext_load(r_prev));
            const int src = c->sc_cur, dst = src ^ 1;
            const size_t ldi = sc_ld(c, c->sc_n), ldo = R::halved_ld(c->sc_n / 2);
            R::fix(c, tab[src], ldi, tab[dst], ldo, c->sc_n, P.t * 8, r);
            R::fix(c, eq[src], ldi, eq[dst], ldo, c->sc_n, 1, r);
            c->sc_cur = dst; c->sc_n /= 2;
        }
        const size_t ld = sc_ld(c, c->sc_n);
        launch_lin_round(R::tab(c), c->desc, tab[c->sc_cur], ld, eq[c->sc_cur], ld, c->sc_n, P.d + 1, partial, od, c->stream());
        c->sc_round++;
        return down_small(c, od, (size_t)(P.d + 2) * RE, evals_out);
    }
    static int sumcheck_lin_end(C *c) {
        std::lock_guard<std::mutex> g(c->mu);
        c->sc_round = -1;
        return LF_OK;
    }
    // ---- the generic sumcheck (lf_mlsumcheck_*, lfhip_sumcheck.h): MLSumcheck::prove_as_subprotocol over any sum of products of MLE tables, split at the
    // transcript like the two above but with a state (ml_*) and buffers (ml_*) of its own; the round kernel is lf_mlsumcheck.hip, the fix between rounds R::fix
    // on the T tables, ping-pong between ml_tab0 and ml_tab1 ----
    // The descriptor's own checks, before the context is looked at: LF_ERR_INVALID first (on what the envelope lets us walk), then the envelope.  *d: the copy
    // the kernel takes, offsets relative to term_off[0], the class of every coefficient per slot
    static int ml_describe(const lf_vpoly *vp, lfml::Desc *d) {
        const u32 q = vp->nterms, T = vp->ntables;
        const bool q_ok = q >= 1 && q <= lfml::MAX_TERMS;
        bool walk = q_ok;   // term_idx can be walked: the offsets increase and span at most MAX_IDX factors
        if (q_ok) {
            for (u32 i = 0; i < q; i++)
                if (vp->term_off[i + 1] <= vp->term_off[i]) return LF_ERR_INVALID;
            walk = vp->term_off[q] <= lfml::MAX_IDX;
            if (walk)
                for (u32 k = vp->term_off[0]; k < vp->term_off[q]; k++)
                    if (vp->term_idx[k] >= T) return LF_ERR_INVALID;
            for (size_t w = 0; w < (size_t)q * RE; w++)
                if (vp->coef[w] >= R::modulus) return LF_ERR_INVALID;
        }
        if (vp->nvars < 1 || vp->nvars > lfml::MAX_NVARS || T < 1 || T > lfml::MAX_TABLES || !walk || vp->degree > lfml::MAX_DEGREE) return LF_ERR_UNSUPPORTED;
        u32 widest = 0;
        for (u32 i = 0; i < q; i++) widest = std::max(widest, vp->term_off[i + 1] - vp->term_off[i]);
        if (widest > lfml::MAX_FACTORS || vp->degree < widest) return LF_ERR_UNSUPPORTED;
        *d = lfml::Desc{};
        d->q = q; d->npts = vp->degree + 1;
        const u32 k0 = vp->term_off[0];
        for (u32 i = 0; i <= q; i++) d->off[i] = vp->term_off[i] - k0;
        for (u32 k = k0; k < vp->term_off[q]; k++) d->set_idx(k - k0, vp->term_idx[k]);
        for (u32 i = 0; i < q; i++)
            for (u32 s = 0; s < 8; s++) {
                const u64 *w = vp->coef + (size_t)i * RE + s * TAU;
                bool tail0 = true;
                for (size_t x = 1; x < TAU; x++) tail0 = tail0 && w[x] == 0;
                const u32 cls = !tail0 ? lfml::COEF_GENERAL : w[0] == 0 ? lfml::COEF_ZERO : w[0] == 1 ? lfml::COEF_ONE : w[0] == R::modulus - 1 ? lfml::COEF_MINUS_ONE : lfml::COEF_GENERAL;
                d->cls[i] |= cls << (2 * s);
            }
        return LF_OK;
    }
    static size_t ml_ld(const C *c, size_t n) { return n == ((size_t)1 << c->ml_nvars) ? n : R::halved_ld(n); }
    // the buffers of a generic sumcheck over T tables of m entries; allocation failure: LF_ERR_HIP
    struct MlBufs { W *tab[2], *coef; Part *partial; u64 *out; };
    static int ml_bufs(C *c, u32 T, size_t m, MlBufs *b) {
        RET(c->tbuf("ml_tab0", (size_t)T * RE * m, &b->tab[0]));
        RET(c->tbuf("ml_tab1", (size_t)T * RE * R::halved_ld(m / 2), &b->tab[1]));
        RET(c->tbuf("ml_coef", (size_t)lfml::MAX_TERMS * RE, &b->coef));
        RET(c->tbuf("ml_partial", lfml::partial_words(R::ml_pts, RE), &b->partial));
        return c->tbuf("ml_out", (size_t)lfml::MAX_TABLES * RE, &b->out);   // (a message is at most 9 elements, the final values at most 16)
    }
    static int mlsumcheck_begin(C *c, const lf_vpoly *vp, const u64 *tables, Origin org = Origin::host) {
        lfml::Desc d;
        RET(ml_describe(vp, &d));
        const u32 T = vp->ntables;
        const size_t m = (size_t)1 << vp->nvars;
        std::lock_guard<std::mutex> g(c->mu);
        if (c->sh_world > 1 || c->xb_on) return LF_ERR_UNSUPPORTED;   // out of scope: one GPU, the default basis
        if (org == Origin::host)
            for (size_t w = 0, nw = (size_t)T * m * RE; w < nw; w++)
                if (tables[w] >= R::modulus) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(tables, (size_t)T * m));
        c->ml_round = -1;   // from here on the buffers of a sumcheck in progress are rewritten: a new one is active only once everything below went through
        MlBufs b;
        RET(ml_bufs(c, T, m, &b));
        RET(io.begin());
        for (u32 j = 0; j < T; j++) RET(up_ring(io, tables + (size_t)j * m * RE, m, b.tab[0] + (size_t)j * RE * m, Form::ntt));
        std::vector<W> hc((size_t)lfml::MAX_TERMS * RE, W(0));
        for (size_t w = 0; w < (size_t)vp->nterms * RE; w++) hc[w] = R::from_canon(vp->coef[w]);
        RET(R::h2d_consts(c, b.coef, hc.data(), hc.size() * sizeof(W)));
        if (io.dev) RET(io.finish());
        else HIPCHK(hipStreamSynchronize(c->stream()));   // the caller's arrays are free again on return
        c->ml_desc = d;
        c->ml_nvars = vp->nvars; c->ml_T = T;
        c->ml_round = 0; c->ml_n = m; c->ml_cur = 0;
        return LF_OK;
    }
    static int mlsumcheck_round(C *c, const u64 *r_prev, u64 *evals_out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (c->ml_round < 0 || c->ml_round >= (int)c->ml_nvars) return LF_ERR_STATE;   // "Prover is not active"
        if ((c->ml_round == 0) != (r_prev == nullptr)) return LF_ERR_STATE;           // "first round should be prover first" / "verifier message is empty"
        HIPCHK(hipSetDevice(c->device));
        const u32 T = c->ml_T;
        MlBufs b;
        RET(ml_bufs(c, T, (size_t)1 << c->ml_nvars, &b));
        if (r_prev) {
            const ExtC r = R::ext_const(c, R::ext_load(r_prev));
            const int src = c->ml_cur, dst = src ^ 1;
            R::fix(c, b.tab[src], ml_ld(c, c->ml_n), b.tab[dst], R::halved_ld(c->ml_n / 2), c->ml_n, T * 8, r);
            c->ml_cur = dst; c->ml_n /= 2;
        }
        if (lfml::launch_mls_round(R::tab(c), c->ml_desc, b.tab[c->ml_cur], ml_ld(c, c->ml_n), c->ml_n / 2, b.coef, b.partial, b.out, c->stream()) != 0) return LF_ERR_HIP;
        c->ml_round++;
        return down_small(c, b.out, (size_t)c->ml_desc.npts * RE, evals_out);
    }
    // after the last round: the last fix, every table's value at the whole point (canonical words, T ring elements)
    static int mlsumcheck_final(C *c, const u64 *r_last, u64 *evals_out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (c->ml_round < 0 || c->ml_round != (int)c->ml_nvars) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        const u32 T = c->ml_T;
        MlBufs b;
        RET(ml_bufs(c, T, (size_t)1 << c->ml_nvars, &b));
        const ExtC r = R::ext_const(c, R::ext_load(r_last));
        R::fix_final(c, b.tab[c->ml_cur], ml_ld(c, c->ml_n), T * 8, r, b.out);   // (two entries are left: the leading dimension is 2 on both rings)
        return down_small(c, b.out, (size_t)T * RE, evals_out);
    }
    static int mlsumcheck_end(C *c) {
        std::lock_guard<std::mutex> g(c->mu);
        c->ml_round = -1;
        return LF_OK;
    }
    // prove_as_subprotocol (utils/sumcheck.rs:53-80): the loop over the split form with the transcript steps of lf_step_host.h.  Everything begin refuses is
    // refused before the first absorb
    static int mlsumcheck_prove(C *c, typename R::Host::Tr &tr, const lf_vpoly *vp, const u64 *tables, u64 *msgs_out, u64 *point_out, u64 *final_out, Origin org) {
        typedef typename R::Host V;
        RET(mlsumcheck_begin(c, vp, tables, org));
        lfs::sumcheck_prologue<V>(tr, vp->nvars, vp->degree);
        const u32 npts = vp->degree + 1;
        const u64 *r_prev = nullptr;
        int rc = LF_OK;
        for (u32 i = 0; i < vp->nvars && rc == LF_OK; i++) {
            u64 *ev = msgs_out + (size_t)i * npts * RE, rw[RE];
            rc = mlsumcheck_round(c, r_prev, ev);
            if (rc != LF_OK) break;
            V::from_ext(lfs::sumcheck_round<V>(tr, ev, npts), rw);   // the challenge as a ring element: every slot carries its tau words
            memcpy(point_out + (size_t)i * TAU, rw, TAU * 8);
            r_prev = point_out + (size_t)i * TAU;
        }
        if (rc == LF_OK && final_out) rc = mlsumcheck_final(c, r_prev, final_out);
        mlsumcheck_end(c);
        return rc;
    }

    // The folding sumcheck with the comb function of nifs/folding/utils.rs:273-325.  `tables` is the reference's mle list of create_sumcheck_polynomial
    // (folding/utils.rs:200-259): [eq(r_L), G_L, eq(r_R), G_R, eq(beta), f-hat_{0,0} .. f-hat_{2K-1,tau-1}], 5 + 2K*tau tables of m ring elements; the three eq
    // tables must be slot-constant (they are diagonal embeddings in the reference).  On the device: T = [eqL, eqR, eqB (tau planes each), G_L, G_R (RE planes each)]
    static constexpr size_t T5P = 3 * TAU + 2 * RE;
    static int sumcheck_fold_begin(C *c, const u64 *tables, const u64 *mu, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        const lf_params &P = c->P;
        const size_t m = c->m;
        const u32 K2 = 2 * P.K;
        static const int eq_idx[3] = {0, 2, 4};
        DevIo<C> io(c, org);
        RET(io.array(tables, (5 + (size_t)K2 * TAU) * m));
        if (!io.dev)   // (device tables: the same test on the device, launch_slot_const_check below)
            for (int e = 0; e < 3; e++) {   // slot-constant check of the eq tables
                const u64 *tb = tables + (size_t)eq_idx[e] * m * RE;
                for (size_t i = 0; i < m; i++)
                    for (size_t sl = 1; sl < 8; sl++)
                        if (memcmp(tb + i * RE, tb + i * RE + TAU * sl, TAU * 8) != 0) return LF_ERR_UNSUPPORTED;
            }
        W *T, *F, *tmp;
        RET(c->tbuf("sf_T0", T5P * m, &T));
        RET(c->tbuf("sf_F0", (size_t)K2 * TAU * RE * m, &F));
        RET(c->tbuf("sf_tmp", RE * m, &tmp));
        RET(io.begin());
        if (io.dev) c->sf_round = -1;   // as in sumcheck_lin_begin
        for (int e = 0; e < 3; e++) {   // eqL, eqR, eqB -> extension-field tables (slot 0 of the ring table); one stream orders tmp's reuse
            RET(up_ring(io, tables + (size_t)eq_idx[e] * m * RE, m, tmp, Form::ntt));
            if (io.dev) launch_slot_const_check(tmp, m, io.flag, c->stream());
            HIPCHK(hipMemcpyAsync(T + TAU * e * m, tmp, TAU * m * sizeof(W), hipMemcpyDeviceToDevice, c->stream()));
        }
        RET(up_ring(io, tables + (size_t)1 * m * RE, m, T + 3 * TAU * m, Form::ntt));
        RET(up_ring(io, tables + (size_t)3 * m * RE, m, T + (3 * TAU + RE) * m, Form::ntt));
        for (u32 i = 0; i < K2 * TAU; i++) RET(up_ring(io, tables + (size_t)(5 + i) * m * RE, m, F + (size_t)i * RE * m, Form::ntt));
        std::vector<ExtC> mu_pow((size_t)K2 * TAU);   // mu_i^1 .. mu_i^tau in the kernels' constant form
        for (u32 i = 0; i < K2; i++) {
            const Ext mi = R::ext_load(mu + TAU * i);
            Ext pm = mi;
            for (size_t d = 0; d < TAU; d++) { mu_pow[(size_t)i * TAU + d] = R::ext_const(c, pm); pm = R::ext_mul(c, pm, mi); }
        }
        ExtC *d_mu;
        RET(upload_consts(c, R::sf_mu, mu_pow, &d_mu));
        if (io.dev) {   // a word >= p: LF_ERR_INVALID; canonical tables whose eq tables are not slot-constant: the host twin's LF_ERR_UNSUPPORTED
            const int rc = io.finish();
            if (rc != LF_OK) return (io.raised() & 1) || rc != LF_ERR_INVALID ? rc : LF_ERR_UNSUPPORTED;
        }
        c->sf_round = 0; c->sf_n = m; c->sf_cur = 0;
        return LF_OK;
    }
    static int sumcheck_fold_round(C *c, const u64 *r_prev, u64 *evals_out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (c->sf_round < 0 || c->sf_round >= (int)c->P.s) return LF_ERR_STATE;   // "Prover is not active" (sumcheck/prover.rs:63)
        if ((c->sf_round == 0) != (r_prev == nullptr)) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        const lf_params &P = c->P;
        const size_t m = c->m;
        const u32 K2 = 2 * P.K;
        W *T[2], *F[2];
        Part *partial;
        u64 *od;
        ExtC *d_mu;
        RET(c->tbuf("sf_T0", T5P * m, &T[0]));
        RET(c->tbuf("sf_T1", T5P * R::halved_ld(m / 2), &T[1]));
        RET(c->tbuf("sf_F0", (size_t)K2 * TAU * RE * m, &F[0]));
        RET(c->tbuf("sf_F1", (size_t)K2 * TAU * RE * R::halved_ld(m / 2), &F[1]));
        RET(c->tbuf(R::sf_mu, (size_t)K2 * TAU + 8, &d_mu));
        RET(c->tbuf("round_partial", R::fold_partial_words(m), &partial));
        RET(c->tbuf("round_out", 5 * RE, &od));
        if (r_prev) {
            const ExtC r = R::ext_const(c, R::ext_load(r_prev));
            const int src = c->sf_cur, dst = src ^ 1;
            const size_t ldi = sc_ld(c, c->sf_n), ldo = R::halved_ld(c->sf_n / 2);
            R::fix(c, T[src], ldi, T[dst], ldo, c->sf_n, 19, r);
            R::fix(c, F[src], ldi, F[dst], ldo, c->sf_n, K2 * TAU * 8, r);
            c->sf_cur = dst; c->sf_n /= 2;
        }
        const size_t n = c->sf_n, ld = sc_ld(c, n);
        const W *t5 = T[c->sf_cur];
        typename R::FoldA a;
        a.eqL = t5; a.eqR = t5 + TAU * ld; a.eqB = t5 + 2 * TAU * ld; a.G1 = t5 + 3 * TAU * ld; a.G2 = t5 + (3 * TAU + RE) * ld;
        a.ld = ld; a.n = n; a.p0 = 0; a.pcnt = n / 2; a.pF0 = 0;
        c->sf_round++;
        if constexpr (R::small_base)
            if (P.b != 2) return sb_fold_round_abi(c, t5, F[c->sf_cur], n, d_mu, evals_out);
        launch_fold_round(R::tab(c), a, F[c->sf_cur], ld, P.K, d_mu, partial, od, c->stream());
        return down_small(c, od, (size_t)(2 * P.b + 1) * RE, evals_out);
    }
    static int sumcheck_fold_end(C *c) {
        std::lock_guard<std::mutex> g(c->mu);
        c->sf_round = -1;
        return LF_OK;
    }

    // ---- witnesses ----
    static int witness_from_coef_table(C *c, const W *coef_dev /* [RE][N] */, lf_witness **out, DevIo<C> *io = nullptr) {
        int32_t *pl;
        const size_t pl_bytes = c->N * RE * 4;
        RET(lf_planes_alloc(R::owner(c), pl_bytes, &pl));   // the recycle pool: a chain in steady state takes the planes its last step gave back
        auto drop = [&] { lf_planes_release(R::owner(c), pl_bytes, pl); };
        int *viol;
        if (c->tbuf("small_dev", 4096, (u64 **)&viol) != LF_OK) { drop(); return LF_ERR_HIP; }
        (void)hipMemsetAsync(viol, 0, 4, c->stream());
        launch_coef_to_i32(coef_dev, pl, c->N, (u32)(c->P.B / 2), viol, c->stream());
        int hv = 0;
        if ((io && io->fetch() != LF_OK) || hipMemcpyAsync(&hv, viol, 4, hipMemcpyDeviceToHost, c->stream()) != hipSuccess ||
            hipStreamSynchronize(c->stream()) != hipSuccess) {
            drop();
            return LF_ERR_HIP;
        }
        if (io && io->bad()) { drop(); return LF_ERR_INVALID; }   // device input with a word >= p: no handle
        // bit 0: a coefficient outside the bound; bit 1 (Goldilocks, B = 2^32): +2^31, which an int32 plane cannot hold.  The BabyBear kernel writes bit 0 only
        // (B <= 2^30), so the one expression serves both rings
        if (hv) { drop(); return (hv & 1) ? LF_ERR_NORM : LF_ERR_UNSUPPORTED; }
        *out = new lf_witness{R::owner(c), pl, c->N, c->device, pl_bytes};
        return LF_OK;
    }
    // Witness::from_w_ccs, arith.rs:230-248: ICRT -> gadget_decompose(B, L); on the calling thread's lane (its stream, its buffers)
    static int witness_from_w_ccs_lane(C *c, const u64 *w_ccs, lf_witness **out, Origin org = Origin::host) {
        DevIo<C> io(c, org);
        RET(io.array(w_ccs, c->P.wit_len));
        W *a, *b, *d;
        RET(c->tbuf("io_a", (size_t)c->P.wit_len * RE, &a));
        RET(c->tbuf("io_b", (size_t)c->P.wit_len * RE, &b));
        RET(c->tbuf("io_c", c->N * RE, &d));
        RET(io.begin());
        RET(up_ring(io, w_ccs, c->P.wit_len, a, Form::ntt));
        launch_icrt_dense(c->d_icrt, a, b, c->P.wit_len, c->stream());
        launch_decompose(b, c->P.wit_len, c->P.B, c->P.L, 0, d, c->stream(), c->digit_mode);
        return witness_from_coef_table(c, d, out, &io);
    }
    static int witness_from_w_ccs(C *c, const u64 *w_ccs, lf_witness **out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        return witness_from_w_ccs_lane(c, w_ccs, out, org);
    }
    static int witness_from_f_coeff(C *c, const u64 *f_coeff, lf_witness **out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(f_coeff, c->N));
        W *d;
        RET(c->tbuf("io_c", c->N * RE, &d));
        RET(io.begin());
        RET(up_ring(io, f_coeff, c->N, d, Form::coeff));
        return witness_from_coef_table(c, d, out, &io);
    }
    static int witness_from_f(C *c, const u64 *f_ntt, lf_witness **out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(f_ntt, c->N));
        W *a, *d;
        RET(c->tbuf("io_a", c->N * RE, &a));
        RET(c->tbuf("io_c", c->N * RE, &d));
        RET(io.begin());
        RET(up_ring(io, f_ntt, c->N, a, Form::ntt));
        launch_icrt_dense(c->d_icrt, a, d, c->N, c->stream());
        return witness_from_coef_table(c, d, out, &io);
    }
    static int witness_get_f_coeff(C *c, const lf_witness *w, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(out, w->N));
        W *d;
        RET(c->tbuf("io_c", w->N * RE, &d));
        launch_i32_to_coef(w->planes, d, w->N, c->stream());
        return down_ring(io, d, w->N, out, Form::coeff);
    }
    static int witness_get_f(C *c, const lf_witness *w, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(out, w->N));
        if (w->f_ntt) return down_ring(io, (const W *)w->f_ntt, w->N, out, Form::ntt);      // built inside the fold step that produced this witness
        W *d, *e;
        RET(c->tbuf("io_c", w->N * RE, &d));
        RET(c->tbuf("io_b", w->N * RE, &e));
        launch_i32_to_coef(w->planes, d, w->N, c->stream());
        launch_crt_fwd(R::tab(c), d, e, w->N, c->stream());
        return down_ring(io, e, w->N, out, Form::ntt);
    }
    static int witness_get_w_ccs(C *c, const lf_witness *w, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(out, c->P.wit_len));
        if (w->w_ccs && w->w_bytes == (size_t)c->P.wit_len * RE * sizeof(W)) return down_ring(io, (const W *)w->w_ccs, c->P.wit_len, out, Form::ntt);
        W *e;
        RET(c->tbuf("io_b", (size_t)c->P.wit_len * RE, &e));
        launch_recompose_crt(R::tab(c), w->planes, w->N, c->P.wit_len, c->P.L, c->P.B, 1, 0, e, c->P.wit_len, 0, c->stream());
        return down_ring(io, e, c->P.wit_len, out, Form::ntt);
    }
    static int witness_commit(C *c, const lf_witness *w, u64 *cm_out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->A_loaded) return LF_ERR_STATE;
        if (w->N != c->nA_total) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        u64 *o;
        RET(c->tbuf("io_o", (size_t)c->kappa * RE, &o));
        c->tn = Tunables::read(R::lut_min_default);
        c->ev_reset();
        RET(commit_dev_i8g(c, nullptr, 0, 1, w->planes + c->A_col0, w->N, o, true));   // timed: lf_last_kernel_stats reports the stand-alone kernel
        c->ev_collect();
        return R::commit_finish(c, o, (size_t)c->kappa * RE, cm_out);   // the sharded gather: per ring
    }

    // ---- decomposed witnesses: decompose_witness (nifs/decomposition.rs:162-167) and its inverse on handles (lf_witness_parts.hip) ----
    // what both directions need of the context, under its lock: a constraint system, and K base-b digits that cover B/2 under the digit rule in force -- the
    // test a decomposition step performs where it starts (the rule may have changed since the load)
    static int parts_ready(const C *c, u32 *lb) {
        if (!c->have_ccs) return LF_ERR_STATE;
        const lf_params &P = c->P;
        if (P.K > lfparts::MAX_PARTS || !sb_digits_cover(P.b, P.K, P.B, c->digit_mode)) return LF_ERR_UNSUPPORTED;
        *lb = sb_log2(P.b);
        return LF_OK;
    }
    // parts_out[k] = Witness::from_f_coeff(part k of decompose_B_vec_into_k_vec(wit.f_coeff)): K handles with planes of their own, so that each is freed alone
    static int witness_decompose(C *c, const lf_witness *wit, lf_witness **parts_out) {
        std::lock_guard<std::mutex> g(c->mu);
        u32 lb;
        const int ready = parts_ready(c, &lb);
        if (ready == LF_ERR_STATE) return ready;
        const u32 K = c->P.K;
        if (wit->N != c->N) return LF_ERR_INVALID;
        RET(ready);
        HIPCHK(hipSetDevice(c->device));
        const size_t bytes = c->N * RE * 4;
        int32_t *pl[lfparts::MAX_PARTS] = {};
        int rc = LF_OK;
        for (u32 k = 0; k < K && rc == LF_OK; k++) rc = lf_planes_alloc(R::owner(c), bytes, &pl[k]);
        if (rc == LF_OK && lfparts::launch_witness_cut(wit->planes, c->N * RE, K, lb, c->digit_mode, pl, c->stream()) != 0) rc = LF_ERR_HIP;
        if (hipStreamSynchronize(c->stream()) != hipSuccess) rc = LF_ERR_HIP;   // (before any of the planes goes back to the pool)
        if (rc != LF_OK) {
            for (u32 k = 0; k < K; k++)
                if (pl[k]) lf_planes_release(R::owner(c), bytes, pl[k]);
            return rc;
        }
        for (u32 k = 0; k < K; k++) parts_out[k] = new lf_witness{R::owner(c), pl[k], c->N, c->device, bytes};
        return LF_OK;
    }
    // *out = the witness whose base-b parts are parts[0..count): digits in the rule's range that are the decomposition of their own sum, a sum the ingest of
    // lf_witness_from_f_coeff accepts.  Anything else is refused with the flag the kernel raised (it rides home in front of the call's only synchronise)
    static int witness_recompose(C *c, const lf_witness *const *parts, unsigned count, lf_witness **out) {
        std::lock_guard<std::mutex> g(c->mu);
        *out = nullptr;
        u32 lb;
        const int ready = parts_ready(c, &lb);
        if (ready == LF_ERR_STATE) return ready;
        if (count != c->P.K) return LF_ERR_INVALID;
        const int32_t *pl[lfparts::MAX_PARTS] = {};
        for (u32 k = 0; k < count; k++) {
            if (!parts[k] || parts[k]->ctx != R::owner(c) || parts[k]->N != c->N) return LF_ERR_INVALID;
            if (k < lfparts::MAX_PARTS) pl[k] = parts[k]->planes;
        }
        RET(ready);
        HIPCHK(hipSetDevice(c->device));
        u32 *flag;
        RET(c->tbuf("small_dev", 4096, (u64 **)&flag));
        const size_t bytes = c->N * RE * 4;
        int32_t *sum;
        RET(lf_planes_alloc(R::owner(c), bytes, &sum));
        u32 hv = 0;
        int rc = LF_OK;
        if (hipMemsetAsync(flag, 0, 4, c->stream()) != hipSuccess ||
            lfparts::launch_witness_join(pl, c->N * RE, count, lb, c->digit_mode, c->P.B / 2, sum, flag, c->stream()) != 0 ||
            hipMemcpyAsync(&hv, flag, 4, hipMemcpyDeviceToHost, c->stream()) != hipSuccess)
            rc = LF_ERR_HIP;
        if (hipStreamSynchronize(c->stream()) != hipSuccess) rc = LF_ERR_HIP;
        if (rc == LF_OK && hv)
            rc = (hv & (lfparts::FLAG_DIGIT | lfparts::FLAG_NOT_CANONICAL)) ? LF_ERR_INVALID : ((hv & lfparts::FLAG_NORM) ? LF_ERR_NORM : LF_ERR_UNSUPPORTED);
        if (rc != LF_OK) { lf_planes_release(R::owner(c), bytes, sum); return rc; }
        *out = new lf_witness{R::owner(c), sum, c->N, c->device, bytes};
        return LF_OK;
    }

    // ---- witness tables (lfhip_tables.h): f-hat, z, M z, M^T v and fix_variables on tables, each ONE body for both spellings ----
    // Order of the refusals, the same for all five: the ABI function's null / foreign-handle checks; here under the lock: a handle with another N ->
    // LF_ERR_INVALID, no constraint system -> LF_ERR_STATE (not for fix_variables), index / count / length / a word >= p -> LF_ERR_INVALID, a sharded context -> LF_ERR_UNSUPPORTED, the pointer and overlap checks of a
    // device array -> LF_ERR_INVALID; only then is anything allocated or enqueued.  None of the calls has a device input but spmv_t and fix_variables, whose
    // results go into the caller's buffer behind the canonical-word flag like every other _dev result
    static bool words_canonical(const u64 *w, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (w[i] >= R::modulus) return false;
        return true;
    }
    // Witness::get_fhat for `count` witnesses: table (w tau + j) of out = f-hat_j of wits[w]; one launch per witness, every word of out written once by it
    static int witness_get_fhat(C *c, const lf_witness *const *wits, unsigned count, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        for (unsigned w = 0; w < count && c->have_ccs; w++)   // (without a constraint system there is no N to compare with)
            if (wits[w]->N != c->N) return LF_ERR_INVALID;
        if (!c->have_ccs) return LF_ERR_STATE;
        if (!count) return LF_ERR_INVALID;
        if (c->sh_world > 1) return LF_ERR_UNSUPPORTED;
        HIPCHK(hipSetDevice(c->device));
        const size_t per = TAU * c->m;   // ring elements per witness
        DevIo<C> io(c, org);
        RET(io.array(out, count * per));
        if (io.dev) {
            for (unsigned w = 0; w < count; w++) launch_fhat(R::tab(c), wits[w]->planes, c->N, c->m, out + w * per * RE, c->stream());
            HIPCHK(hipStreamSynchronize(c->stream()));
            return LF_OK;
        }
        u64 *tmp;
        RET(c->tbuf("stage_aos", per * RE, &tmp));
        for (unsigned w = 0; w < count; w++) {   // (one stream: the next launch overwrites the stage only after the copy before it)
            launch_fhat(R::tab(c), wits[w]->planes, c->N, c->m, tmp, c->stream());
            HIPCHK(hipMemcpyAsync(out + w * per * RE, tmp, per * RE * 8, hipMemcpyDeviceToHost, c->stream()));
        }
        HIPCHK(hipStreamSynchronize(c->stream()));
        return LF_OK;
    }
    // z = x || 1 || w_ccs of a witness as the plane table [RE][n] the SpMV launchers read (buffer "tab_z"); x: l elements, host, internal basis, canonical
    static int z_planes(C *c, const lf_witness *w, const u64 *x, W **z_out) {
        const size_t l = c->P.l, wl = c->P.wit_len, n = c->n;
        W *z;
        u64 *xs;
        RET(c->tbuf("tab_z", n * RE, &z));
        RET(c->tbuf("tab_x", (l + 1) * RE, &xs));
        if (l) HIPCHK(hipMemcpyAsync(xs, x, l * RE * 8, hipMemcpyHostToDevice, c->stream()));
        launch_z_head(xs, l, z, n, c->stream());
        if (w->w_ccs && w->w_bytes == wl * RE * sizeof(W))   // materialised by the fold step that made this witness: planes [RE][wit_len]
            HIPCHK(hipMemcpy2DAsync(z + l + 1, n * sizeof(W), w->w_ccs, wl * sizeof(W), wl * sizeof(W), RE, hipMemcpyDeviceToDevice, c->stream()));
        else launch_recompose_crt(R::tab(c), w->planes, w->N, (u32)wl, c->P.L, c->P.B, 1, 0, z, n, l + 1, c->stream());
        *z_out = z;
        return LF_OK;
    }
    static int witness_tables_ready(C *c, const lf_witness *w, const u64 *x) {
        if (c->have_ccs && w->N != c->N) return LF_ERR_INVALID;
        if (!c->have_ccs) return LF_ERR_STATE;
        if (!words_canonical(x, (size_t)c->P.l * RE)) return LF_ERR_INVALID;
        return c->sh_world > 1 ? LF_ERR_UNSUPPORTED : LF_OK;
    }
    static int witness_get_z(C *c, const lf_witness *w, const u64 *x, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        RET(witness_tables_ready(c, w, x));
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(out, c->n));
        W *z;
        RET(z_planes(c, w, x, &z));
        return down_ring(io, z, c->n, out, Form::ntt);
    }
    // calculate_Mz_mles (utils/mle_helpers.rs:137-146): table j of out = M_j z, one SpMV launch per matrix as lf_spmv runs it; on Goldilocks over the live rows
    // only (lf_live_rows.h: the rows behind them are zeros of every M_j z -- one memset)
    static int witness_mz(C *c, const lf_witness *w, const u64 *x, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        RET(witness_tables_ready(c, w, x));
        HIPCHK(hipSetDevice(c->device));
        const size_t m = c->m, n = c->n;
        const u32 t = c->P.t;
        DevIo<C> io(c, org);
        RET(io.array(out, t * m));
        W *z, *od;
        RET(c->tbuf("tab_mz", (size_t)t * RE * m, &od));
        RET(z_planes(c, w, x, &z));
        if constexpr (R::general_csr) {
            const size_t live = c->live_rows < m ? c->live_rows : m;
            W *zaos = nullptr;
            if (c->ccs_general) RET(c->tbuf("spmv_zaos", n * RE, &zaos));
            if (live < m) HIPCHK(hipMemsetAsync(od, 0, (size_t)t * RE * m * sizeof(W), c->stream()));
            for (u32 j = 0; j < t; j++) {
                W *oj = od + (size_t)j * RE * m;
                if (c->ccs_general)   // (the element-major copy of z is made by the first launch and read by the others)
                    launch_spmv_rows(R::tab(c), 1, &c->d_rowptr[j], &c->d_col[j], &c->d_val[j], j ? nullptr : z, 0, n, zaos, oj, m, 0, c->stream(), 0, live);
                else launch_spmv(R::tab(c), c->d_rowptr[j], c->d_col[j], c->d_val[j], z, n, oj, m, 0, c->stream(), 0, live);
            }
        } else {
            for (u32 j = 0; j < t; j++) launch_spmv(R::tab(c), c->d_rowptr[j], c->d_col[j], c->d_val[j], z, n, od + (size_t)j * RE * m, m, 0, c->stream());
        }
        if (io.dev) {
            for (u32 j = 0; j < t; j++) store_ring(io, od + (size_t)j * RE * m, m, out + (size_t)j * m * RE, Form::ntt);
            return io.finish();
        }
        for (u32 j = 0; j < t; j++) RET(down_ring(c, od + (size_t)j * RE * m, m, out + (size_t)j * m * RE, Form::ntt));
        return LF_OK;
    }
    // out (n elements) = M_j^T v, v = m general ring elements (lf_spmv_t.cuh)
    static int spmv_t(C *c, unsigned j, const u64 *v, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        if (j >= c->P.t) return LF_ERR_INVALID;
        if (c->sh_world > 1) return LF_ERR_UNSUPPORTED;
        if (org == Origin::host && !words_canonical(v, c->m * RE)) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(v, c->m));
        RET(io.array(out, c->n));
        RET(io.disjoint(v, c->m, out, c->n));
        W *vw, *od, *part;
        RET(c->tbuf("io_a", c->m * RE, &vw));
        RET(c->tbuf("io_b", c->n * RE, &od));
        RET(c->tbuf("spmvt_part", (size_t)c->spmvt_items[j] * RE + 8, &part));
        RET(io.begin());
        const u64 *src = v;
        if (!io.dev) {
            u64 *tmp;
            RET(c->tbuf("stage_aos", c->m * RE, &tmp));
            HIPCHK(hipMemcpyAsync(tmp, v, c->m * RE * 8, hipMemcpyHostToDevice, c->stream()));
            src = tmp;
        }
        const auto Ti = R::xb_mat(c->xb_Ti);
        launch_aos_words(src, vw, c->m, c->stream(), io.flag, xb_converts(c, Form::ntt) ? &Ti : nullptr);
        launch_spmv_t(R::tab(c), c->d_colptr[j], c->d_rowidx[j], c->d_valT[j], vw, od, c->n, c->spmvt_min, c->d_spmvt_plan[j], c->spmvt_items[j], c->spmvt_cols[j],
                      part, c->stream());
        return down_ring(io, od, c->n, out, Form::ntt);
    }
    // DenseMultilinearExtension::fix_variables on `ntables` tables of len = 2^nv entries: the lowest nfix variables, one R::fix per variable, ping-pong between two
    // scratch tables (leading dimensions as in the generic sumcheck); works on a bare context
    static int mle_fix_variables(C *c, const u64 *tables, size_t ntables, size_t len, const u64 *point, unsigned nfix, u64 *out, Origin org = Origin::host) {
        if (!ntables || len < 2 || (len & (len - 1)) || !nfix || nfix >= 64 || ((size_t)1 << nfix) > len) return LF_ERR_INVALID;
        if (!words_canonical(point, (size_t)nfix * TAU)) return LF_ERR_INVALID;
        std::lock_guard<std::mutex> g(c->mu);
        if (c->sh_world > 1) return LF_ERR_UNSUPPORTED;
        if (org == Origin::host && !words_canonical(tables, ntables * len * RE)) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        const size_t len_out = len >> nfix;
        DevIo<C> io(c, org);
        RET(io.array(tables, ntables * len));
        RET(io.array(out, ntables * len_out));
        RET(io.disjoint(tables, ntables * len, out, ntables * len_out));
        W *tab[2];
        RET(c->tbuf("fx_tab0", ntables * RE * len, &tab[0]));
        RET(c->tbuf("fx_tab1", ntables * RE * R::halved_ld(len / 2), &tab[1]));
        RET(io.begin());
        for (size_t a = 0; a < ntables; a++) RET(up_ring(io, tables + a * len * RE, len, tab[0] + a * RE * len, Form::ntt));
        size_t n = len, ld = len;
        int cur = 0;
        for (unsigned i = 0; i < nfix; i++) {
            const ExtC r = R::ext_const(c, R::ext_load(point + TAU * i));
            const size_t ldo = R::halved_ld(n / 2);
            for (size_t a0 = 0; a0 < ntables; a0 += 4096) {   // (a launch takes rows in its grid's y: at most 65535 / 8 tables at a time)
                const size_t na = ntables - a0 < 4096 ? ntables - a0 : 4096;
                R::fix(c, tab[cur] + a0 * RE * ld, ld, tab[cur ^ 1] + a0 * RE * ldo, ldo, n, (u32)(na * 8), r);
            }
            cur ^= 1; n /= 2; ld = ldo;
        }
        const W *res = tab[cur];
        if (ld != n) {   // (a leading dimension padded beyond the length: the planes move together for the relayout, which takes ld == n)
            HIPCHK(hipMemcpy2DAsync(tab[cur ^ 1], n * sizeof(W), tab[cur], ld * sizeof(W), n * sizeof(W), ntables * RE, hipMemcpyDeviceToDevice, c->stream()));
            res = tab[cur ^ 1];
        }
        if (io.dev) {
            for (size_t a = 0; a < ntables; a++) store_ring(io, res + a * RE * n, n, out + a * n * RE, Form::ntt);
            return io.finish();
        }
        for (size_t a = 0; a < ntables; a++) RET(down_ring(c, res + a * RE * n, n, out + a * n * RE, Form::ntt));
        return LF_OK;
    }

    // ---- folding helpers ----
    // compute_f_0 (nifs/folding.rs:258-268): out[j] = sum_i coef_i (.) tables_i[j] with ring-element coefficients (8 distinct slots)
    static int lincomb(C *c, const u64 *coef, const u64 *tables, size_t n_terms, size_t len, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        DevIo<C> io(c, org);
        RET(io.array(tables, n_terms * len));
        RET(io.array(out, len));
        RET(io.disjoint(tables, n_terms * len, out, len));
        W *X, *o;
        RET(c->tbuf("io_a", n_terms * len * RE, &X));
        RET(c->tbuf("io_b", len * RE, &o));
        RET(io.begin());
        for (size_t i = 0; i < n_terms; i++) RET(up_ring(io, tables + i * len * RE, len, X + i * RE * len, Form::ntt));
        std::vector<ExtC> cf(n_terms * 8);
        for (size_t i = 0; i < n_terms; i++)
            for (size_t sl = 0; sl < 8; sl++) cf[i * 8 + sl] = R::ext_const(c, R::ext_load(coef + i * RE + TAU * sl));
        ExtC *d_cf;
        RET(upload_consts(c, "lc_coef", cf, &d_cf));
        launch_lincomb_z(R::tab(c), X, len, (u32)n_terms, d_cf, 1, len, o, c->stream(), 1);
        return down_ring(io, o, len, out, Form::ntt);
    }
    // calculate_challenged_mz_mle (nifs/folding.rs:208-226) and the f-hat half of prepare_g1_and_3_k_mles_list (folding/utils.rs:524-546):
    // out[x] = sum_{i<groups} sum_{j<per_group} c_i^{j+1} T_{i,j}[x] (the reference's Horner loop `mle += M; mle *= c_i` over j reversed)
    static int horner_combine(C *c, const u64 *tables, size_t groups, size_t per_group, size_t len, const u64 *challenges, u64 *out, Origin org = Origin::host) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        const size_t nt = groups * per_group;
        DevIo<C> io(c, org);
        RET(io.array(tables, nt * len));
        RET(io.array(out, len));
        RET(io.disjoint(tables, nt * len, out, len));
        W *X, *o;
        RET(c->tbuf("io_a", nt * len * RE, &X));
        RET(c->tbuf("io_b", len * RE, &o));
        RET(io.begin());
        for (size_t i = 0; i < nt; i++) RET(up_ring(io, tables + i * len * RE, len, X + i * RE * len, Form::ntt));
        std::vector<ExtC> cf(nt);
        for (size_t i = 0; i < groups; i++) {
            Ext ci = R::ext_load(challenges + TAU * i), pw = ci;
            for (size_t j = 0; j < per_group; j++) { cf[i * per_group + j] = R::ext_const(c, pw); pw = R::ext_mul(c, pw, ci); }
        }
        ExtC *d_cf;
        RET(upload_consts(c, "lc_coef", cf, &d_cf));
        launch_lincomb_z(R::tab(c), X, len, (u32)nt, d_cf, 1, len, o, c->stream(), 0);
        return down_ring(io, o, len, out, Form::ntt);
    }
};
}  // namespace lfring
using lfring::BbRing;
using lfring::GoldRing;
using lfring::ring_ops;
// the staging and commit helpers the provers of both backends call (unqualified, from the global namespace and from lfbb)
using lfring::commit_dev_i8g;
using lfring::i8_rc;
using lfring::commit_dev_pre;
using lfring::commit_planes_i8;
using lfring::DevIo;
using lfring::down_ring;
using lfring::Form;
using lfring::Origin;
using lfring::pow2;
using lfring::up_ring;
using lfring::upload_consts;
using lfring::witness_commit_dev;
#pragma GCC visibility pop
