// lf_ring_host.h -- the host side of the ring-generic entry points, ONCE for both rings (the pattern of poseidon_host.h): a small policy per ring
// (GoldRing: lf_ctx, 24 canonical u64 words, tau 3; BbRing: lfbb::BbCtxImpl, 72 centred Montgomery int32 words, tau 9) and one template per body.
// The launchers are NOT wrapped: lf:: and lfbb:: declare them as overload sets over the word type and the table struct, and both namespaces are
// visible below, so a call resolves by the types the policy hands out.  Context members that carry the same name on both rings (mu, device, stream(),
// tbuf, ring, d_icrt, P, N, m, n, kappa, nA, ...) are used directly.  lf_capi.cpp keeps the argument checks, the external-basis wrapper and the
// dispatch `c->bb ? ring_ops<BbRing>::f(c->bb->p, ..) : ring_ops<GoldRing>::f(c, ..)`.
//
// Stays per backend (really different, not copies): build_eq_dev / build_eq_async (two-level kernel against pre-multiplied constants), build_z,
// lcccs_point, install_tables, ccs_load, ajtai_load / ajtai_generate / prep_ajtai_i8*, the lf_ajtai_commit* and ajtai_commit_gadget bodies (their sharded
// finishes differ), selftest_field, down_small (per-lane pinned buffer + lane_sync() against one buffer + stream sync), the sumcheck state machines, the
// provers (lf_prove.cpp, lf_fold.cpp, lf_fold_sb.cpp, bb_prove.cpp), lf_dist.cpp, the verifier, the wire format and lfp_*.
//
// Order of the argument checks, the same on both rings: (1) null / range checks of the ABI function -> LF_ERR_INVALID, (2) here, before the context
// lock: pow2(base) -> LF_ERR_UNSUPPORTED (decompose), len against 2^nv -> LF_ERR_INVALID (mle_eval_batch), (3) under the lock: have_ccs / resident
// matrix -> LF_ERR_STATE, then index and length checks -> LF_ERR_INVALID.
#pragma once
#include "bb_ctx.h"
#include "lf_check.h"
#include "lf_ctx.h"

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
    static constexpr int RE = 24, TAU = 3;
    static constexpr bool general_csr = true;    // ccs_general / launch_spmv_rows exist on this ring only
    static constexpr bool montgomery = false;
    static constexpr const char *mle_out = "io_b", *i8g_co = "i8g_coef";
    static const DevCrt &tab(const lf_ctx *c) { return c->dcrt; }
    static bool have_A(const lf_ctx *c) { return c->A_loaded; }
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
    static constexpr int RE = lfbb::RE, TAU = lfbb::TAU;
    static constexpr bool general_csr = false;
    static constexpr bool montgomery = true;
    static constexpr const char *mle_out = "io_o", *i8g_co = "i8g_co";
    static const DevBb &tab(const BbCtxImpl *c) { return c->dev; }
    static bool have_A(const BbCtxImpl *c) { return c->dAb != nullptr; }
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
// upload n ring elements (AoS) into a plane table dst [RE][n]
template <class C>
int up_ring(C *c, const u64 *host, size_t n, typename Ring<C>::W *dst) {
    if (!n) return LF_OK;
    u64 *tmp;
    RET(c->tbuf("stage_aos", n * Ring<C>::RE, &tmp));
    HIPCHK(hipMemcpyAsync(tmp, host, n * Ring<C>::RE * 8, hipMemcpyHostToDevice, c->stream()));
    launch_aos_to_soa(tmp, dst, n, c->stream());
    return LF_OK;
}
template <class C>
int down_ring(C *c, const typename Ring<C>::W *src, size_t n, u64 *host) {
    if (!n) return LF_OK;
    u64 *tmp;
    RET(c->tbuf("stage_aos", n * Ring<C>::RE, &tmp));
    launch_soa_to_aos(src, tmp, n, c->stream());
    HIPCHK(hipMemcpyAsync(host, tmp, n * Ring<C>::RE * 8, hipMemcpyDeviceToHost, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));
    return LF_OK;
}
template <class C, class T>
int upload_consts(C *c, const std::string &name, const std::vector<T> &v, T **out) {
    RET(c->tbuf(name, v.size() + 8, out));
    return Ring<C>::h2d_consts(c, *out, v.data(), v.size() * sizeof(T));
}

// ---- general commit, host side -----------------------------------------------------------------------------------------------------------------------
// The contraction of `batch` operands whose digit words [NP][RE][ntiles] of this rank's columns the caller's pass cut(b, pre, ntiles) writes: NP = 10 (5 on
// BabyBear) for an arbitrary element, 5 for the int32 planes of a witness handle, fewer for the digits of a gadget decomposition (ajtai_i8g_planes_base).
// out_dev: canonical u64 [batch][kappa][RE] NTT form, AoS (PARTIAL when sharded).
template <class C, class Cut>
int commit_dev_pre(C *c, u32 NP, u32 batch, u64 *out_dev, bool timed, Cut &&cut) {
    typedef Ring<C> R;
    typedef typename R::W W;
    if (!R::have_A(c) || !c->i8_nch || !c->dAb) return LF_ERR_STATE;
    const AjtaiI8Ring I = R::i8();
    const u32 nch = c->i8_nch, kc = c->i8_kc, MT = ajtai_i8_row_tiles(I, kc);
    const size_t ntiles = (c->nA + 7) / 8, chunk_bytes = ntiles * (I.RD / 8) * MT * 1024;
    const char *e_wgs = getenv("LF_I8G_WGS");           // (test hook: workgroups of the general commit kernel; default one per CU)
    const u32 nwg = e_wgs && atoi(e_wgs) > 0 ? (u32)atoi(e_wgs) : 256;
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
            const int g = launch_ajtai_i8g(I, c->dAb + (size_t)ch * chunk_bytes, MT, pre, ntiles, c->nA, kn, row0, c->kappa, NP, nwg, part, dsum, sum, co, c->stream());
            if (g < 0) return LF_ERR_UNSUPPORTED;
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

    // ---- a1/a2/a3 ----
    static int ntt_fwd(C *c, const u64 *in, u64 *out, size_t count) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *a, *b;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * RE, &b));
        RET(up_ring(c, in, count, a));
        launch_crt_fwd(R::tab(c), a, b, count, c->stream());
        return down_ring(c, b, count, out);
    }
    static int ntt_inv(C *c, const u64 *in, u64 *out, size_t count) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *a, *b;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * RE, &b));
        RET(up_ring(c, in, count, a));
        launch_icrt_dense(c->d_icrt, a, b, count, c->stream());
        return down_ring(c, b, count, out);
    }
    static int decompose(C *c, const u64 *in, size_t count, u64 base, unsigned digits, int layout, u64 *out) {
        if (!pow2(base)) return LF_ERR_UNSUPPORTED;
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *a, *b;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * digits * RE, &b));
        RET(up_ring(c, in, count, a));
        launch_decompose(a, count, base, digits, layout, b, c->stream(), c->digit_mode);
        if (layout == 0) return down_ring(c, b, count * digits, out);
        for (unsigned k = 0; k < digits; k++) RET(down_ring(c, b + (size_t)k * RE * count, count, out + (size_t)k * count * RE));
        return LF_OK;
    }
    static int recompose(C *c, const u64 *in, size_t count_out, u64 base, unsigned digits, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *a, *b;
        RET(c->tbuf("io_a", count_out * digits * RE, &a));
        RET(c->tbuf("io_b", count_out * RE, &b));
        RET(up_ring(c, in, count_out * digits, a));
        launch_recompose(a, count_out, base, digits, b, c->stream());
        return down_ring(c, b, count_out, out);
    }
    static int linf_check(C *c, const u64 *f_ntt, size_t count, u64 bound, int unsigned_variant, int *ok, u64 *max_out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *a, *b;
        u64 *mx;
        RET(c->tbuf("io_a", count * RE, &a));
        RET(c->tbuf("io_b", count * RE, &b));
        RET(c->tbuf("small_dev", 4096, &mx));
        RET(up_ring(c, f_ntt, count, a));
        launch_icrt_dense(c->d_icrt, a, b, count, c->stream());
        u64 m = 0;
        if (unsigned_variant) {
            // literal Witness::within_bound (arith.rs:372-386): canonical coefficient < bound.  The maximum is taken over CANONICAL words, so the table comes
            // down through down_ring (BabyBear planes hold Montgomery words); a maximum does not depend on the layout
            std::vector<u64> h(count * RE);
            RET(down_ring(c, b, count, h.data()));
            for (u64 v : h) m = v > m ? v : m;
        } else {
            launch_linf(b, count, mx, c->stream());
            RET(down_small(c, mx, 1, &m));
        }
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
    static int build_eq(C *c, const u64 *point, unsigned nv, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        const size_t n = (size_t)1 << nv;
        W *eq;
        RET(c->tbuf("io_a", TAU * n, &eq));
        RET(build_eq_dev(c, load_point(point, nv).data(), nv, eq));
        std::vector<W> h(TAU * n);
        HIPCHK(hipMemcpyAsync(h.data(), eq, h.size() * sizeof(W), hipMemcpyDeviceToHost, c->stream()));
        HIPCHK(hipStreamSynchronize(c->stream()));
        for (size_t i = 0; i < n; i++)
            for (size_t q = 0; q < TAU; q++) out[TAU * i + q] = R::canon(h[q * n + i]);
        return LF_OK;
    }
    static int mle_eval_batch(C *c, const u64 *tables, size_t ntables, size_t len, const u64 *point, unsigned nv, u64 *out) {
        const size_t n = (size_t)1 << nv;
        if (len > n || len == 0) return LF_ERR_INVALID;   // MleEvaluationError::IncorrectLength
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *eq, *X;
        Part *partial;
        u64 *o;
        RET(c->tbuf("io_eq", TAU * n, &eq));
        RET(c->tbuf("io_a", ntables * len * RE, &X));
        RET(c->tbuf("red_partial", R::red_partial(ntables * RE), &partial));
        RET(c->tbuf(R::mle_out, ntables * RE, &o));   // (the rings name this buffer differently; kept: buffer names are part of a context's memory footprint)
        RET(build_eq_dev(c, load_point(point, nv).data(), nv, eq));
        for (size_t a = 0; a < ntables; a++) RET(up_ring(c, tables + a * len * RE, len, X + a * RE * len));
        launch_dot_eq(R::tab(c), X, len, (u32)ntables, eq, n, len, partial, o, c->stream());
        return down_small(c, o, ntables * RE, out);
    }
    static int spmv(C *c, unsigned j, const u64 *z, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        if (j >= c->P.t) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        W *zd, *od;
        RET(c->tbuf("io_a", c->n * RE, &zd));
        RET(c->tbuf("io_b", c->m * RE, &od));
        RET(up_ring(c, z, c->n, zd));
        if constexpr (R::general_csr) {   // Goldilocks only: dense rows gather whole elements from an element-major z
            if (c->ccs_general) {
                W *zaos;
                RET(c->tbuf("spmv_zaos", c->n * RE, &zaos));
                launch_spmv_rows(R::tab(c), 1, &c->d_rowptr[j], &c->d_col[j], &c->d_val[j], zd, 0, c->n, zaos, od, c->m, 0, c->stream());
                return down_ring(c, od, c->m, out);
            }
        }
        launch_spmv(R::tab(c), c->d_rowptr[j], c->d_col[j], c->d_val[j], zd, c->n, od, c->m, 0, c->stream());
        return down_ring(c, od, c->m, out);
    }

    // ---- witnesses ----
    static int witness_from_coef_table(C *c, const W *coef_dev /* [RE][N] */, lf_witness **out) {
        int32_t *pl;
        HIPCHK(lf_dev_malloc(&pl, c->N * RE * 4));
        int *viol;
        if (c->tbuf("small_dev", 4096, (u64 **)&viol) != LF_OK) { (void)hipFree(pl); return LF_ERR_HIP; }
        (void)hipMemsetAsync(viol, 0, 4, c->stream());
        launch_coef_to_i32(coef_dev, pl, c->N, (u32)(c->P.B / 2), viol, c->stream());
        int hv = 0;
        if (hipMemcpyAsync(&hv, viol, 4, hipMemcpyDeviceToHost, c->stream()) != hipSuccess || hipStreamSynchronize(c->stream()) != hipSuccess) {
            (void)hipFree(pl);
            return LF_ERR_HIP;
        }
        // bit 0: a coefficient outside the bound; bit 1 (Goldilocks, B = 2^32): +2^31, which an int32 plane cannot hold.  The BabyBear kernel writes bit 0 only
        // (B <= 2^30), so the one expression serves both rings
        if (hv) { (void)hipFree(pl); return (hv & 1) ? LF_ERR_NORM : LF_ERR_UNSUPPORTED; }
        *out = new lf_witness{R::owner(c), pl, c->N, c->device, c->N * RE * 4};
        return LF_OK;
    }
    // Witness::from_w_ccs, arith.rs:230-248: ICRT -> gadget_decompose(B, L); on the calling thread's lane (its stream, its buffers)
    static int witness_from_w_ccs_lane(C *c, const u64 *w_ccs, lf_witness **out) {
        W *a, *b, *d;
        RET(c->tbuf("io_a", (size_t)c->P.wit_len * RE, &a));
        RET(c->tbuf("io_b", (size_t)c->P.wit_len * RE, &b));
        RET(c->tbuf("io_c", c->N * RE, &d));
        RET(up_ring(c, w_ccs, c->P.wit_len, a));
        launch_icrt_dense(c->d_icrt, a, b, c->P.wit_len, c->stream());
        launch_decompose(b, c->P.wit_len, c->P.B, c->P.L, 0, d, c->stream(), c->digit_mode);
        return witness_from_coef_table(c, d, out);
    }
    static int witness_from_w_ccs(C *c, const u64 *w_ccs, lf_witness **out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        return witness_from_w_ccs_lane(c, w_ccs, out);
    }
    static int witness_from_f_coeff(C *c, const u64 *f_coeff, lf_witness **out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        W *d;
        RET(c->tbuf("io_c", c->N * RE, &d));
        RET(up_ring(c, f_coeff, c->N, d));
        return witness_from_coef_table(c, d, out);
    }
    static int witness_from_f(C *c, const u64 *f_ntt, lf_witness **out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        W *a, *d;
        RET(c->tbuf("io_a", c->N * RE, &a));
        RET(c->tbuf("io_c", c->N * RE, &d));
        RET(up_ring(c, f_ntt, c->N, a));
        launch_icrt_dense(c->d_icrt, a, d, c->N, c->stream());
        return witness_from_coef_table(c, d, out);
    }
    static int witness_get_f_coeff(C *c, const lf_witness *w, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *d;
        RET(c->tbuf("io_c", w->N * RE, &d));
        launch_i32_to_coef(w->planes, d, w->N, c->stream());
        return down_ring(c, d, w->N, out);
    }
    static int witness_get_f(C *c, const lf_witness *w, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        if (w->f_ntt) return down_ring(c, (const W *)w->f_ntt, w->N, out);      // built inside the fold step that produced this witness
        W *d, *e;
        RET(c->tbuf("io_c", w->N * RE, &d));
        RET(c->tbuf("io_b", w->N * RE, &e));
        launch_i32_to_coef(w->planes, d, w->N, c->stream());
        launch_crt_fwd(R::tab(c), d, e, w->N, c->stream());
        return down_ring(c, e, w->N, out);
    }
    static int witness_get_w_ccs(C *c, const lf_witness *w, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->have_ccs) return LF_ERR_STATE;
        HIPCHK(hipSetDevice(c->device));
        if (w->w_ccs && w->w_bytes == (size_t)c->P.wit_len * RE * sizeof(W)) return down_ring(c, (const W *)w->w_ccs, c->P.wit_len, out);
        W *e;
        RET(c->tbuf("io_b", (size_t)c->P.wit_len * RE, &e));
        launch_recompose_crt(R::tab(c), w->planes, w->N, c->P.wit_len, c->P.L, c->P.B, 1, 0, e, c->P.wit_len, 0, c->stream());
        return down_ring(c, e, c->P.wit_len, out);
    }
    static int witness_commit(C *c, const lf_witness *w, u64 *cm_out) {
        std::lock_guard<std::mutex> g(c->mu);
        if (!R::have_A(c)) return LF_ERR_STATE;
        if (w->N != c->nA_total) return LF_ERR_INVALID;
        HIPCHK(hipSetDevice(c->device));
        u64 *o;
        RET(c->tbuf("io_o", (size_t)c->kappa * RE, &o));
        c->ev_reset();
        RET(commit_dev_i8g(c, nullptr, 0, 1, w->planes + c->A_col0, w->N, o, true));   // timed: lf_last_kernel_stats reports the stand-alone kernel
        c->ev_collect();
        return R::commit_finish(c, o, (size_t)c->kappa * RE, cm_out);   // the sharded gather: per ring
    }

    // ---- folding helpers ----
    // compute_f_0 (nifs/folding.rs:258-268): out[j] = sum_i coef_i (.) tables_i[j] with ring-element coefficients (8 distinct slots)
    static int lincomb(C *c, const u64 *coef, const u64 *tables, size_t n_terms, size_t len, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        W *X, *o;
        RET(c->tbuf("io_a", n_terms * len * RE, &X));
        RET(c->tbuf("io_b", len * RE, &o));
        for (size_t i = 0; i < n_terms; i++) RET(up_ring(c, tables + i * len * RE, len, X + i * RE * len));
        std::vector<ExtC> cf(n_terms * 8);
        for (size_t i = 0; i < n_terms; i++)
            for (size_t sl = 0; sl < 8; sl++) cf[i * 8 + sl] = R::ext_const(c, R::ext_load(coef + i * RE + TAU * sl));
        ExtC *d_cf;
        RET(upload_consts(c, "lc_coef", cf, &d_cf));
        launch_lincomb_z(R::tab(c), X, len, (u32)n_terms, d_cf, 1, len, o, c->stream(), 1);
        return down_ring(c, o, len, out);
    }
    // calculate_challenged_mz_mle (nifs/folding.rs:208-226) and the f-hat half of prepare_g1_and_3_k_mles_list (folding/utils.rs:524-546):
    // out[x] = sum_{i<groups} sum_{j<per_group} c_i^{j+1} T_{i,j}[x] (the reference's Horner loop `mle += M; mle *= c_i` over j reversed)
    static int horner_combine(C *c, const u64 *tables, size_t groups, size_t per_group, size_t len, const u64 *challenges, u64 *out) {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(hipSetDevice(c->device));
        const size_t nt = groups * per_group;
        W *X, *o;
        RET(c->tbuf("io_a", nt * len * RE, &X));
        RET(c->tbuf("io_b", len * RE, &o));
        for (size_t i = 0; i < nt; i++) RET(up_ring(c, tables + i * len * RE, len, X + i * RE * len));
        std::vector<ExtC> cf(nt);
        for (size_t i = 0; i < groups; i++) {
            Ext ci = R::ext_load(challenges + TAU * i), pw = ci;
            for (size_t j = 0; j < per_group; j++) { cf[i * per_group + j] = R::ext_const(c, pw); pw = R::ext_mul(c, pw, ci); }
        }
        ExtC *d_cf;
        RET(upload_consts(c, "lc_coef", cf, &d_cf));
        launch_lincomb_z(R::tab(c), X, len, (u32)nt, d_cf, 1, len, o, c->stream(), 0);
        return down_ring(c, o, len, out);
    }
};
}  // namespace lfring
using lfring::BbRing;
using lfring::GoldRing;
using lfring::ring_ops;
// the staging and commit helpers the provers of both backends call (unqualified, from the global namespace and from lfbb)
using lfring::commit_dev_i8g;
using lfring::commit_dev_pre;
using lfring::down_ring;
using lfring::pow2;
using lfring::up_ring;
using lfring::upload_consts;
using lfring::witness_commit_dev;
#pragma GCC visibility pop
