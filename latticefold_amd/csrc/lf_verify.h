// lf_verify.h -- host-side NIFSVerifier::verify (crates/latticefold/src/nifs.rs:117-163) for either ring, behind
// lf_verify_host (include/lfhip.h).  O(proof size) work, no GPU.  SURVEY 8(f) rank 3: "the step after the path".
//
// Restates: LFLinearizationVerifier::verify (nifs/linearization.rs:264-290, :193-243), LFDecompositionVerifier::verify
// (nifs/decomposition.rs:94-157), LFFoldingVerifier::verify (nifs/folding.rs:136-195, :273-343; expected value
// folding/utils.rs:366-413; outputs folding/utils.rs:460-521), MLSumcheck::verify_as_subprotocol +
// check_and_generate_subclaim + interpolate_uni_poly (utils/sumcheck.rs:82-110, utils/sumcheck/verifier.rs:92-257).
//
// `V` is the ring's host policy (GoldV in lf_host.h, BbV in bb_host.h).  The transcript steps and the instance arithmetic the verifier has in common with the
// provers -- sumcheck transcript, public input, challenge draws, get_rhos, the folded instance -- are the bodies of lf_step_host.h; the checks are here.
#pragma once
#include "lf_step_host.h"

namespace lfv {

typedef uint64_t u64;
typedef uint32_t u32;

// ---- MLSumcheck::verify_as_subprotocol (utils/sumcheck.rs:84-104) on its own: what the NIFS verifier below and lf_mlsumcheck_verify (lfhip_sumcheck.h) share ----
// Lagrange interpolation through (0, p_0), .., (len-1, p_{len-1}) evaluated at `at` (ring elements, slot-constant weights): interpolate_uni_poly
// (utils/sumcheck/verifier.rs:139-257)
template <class V>
void interpolate_uni_poly(const V &v, const u64 *p_i, u32 len, typename V::Ext at, u64 *out) {
    typedef typename V::Ext Ext;
    constexpr int RE = V::RE;
    u64 res[RE] = {0}, t[RE];
    for (u32 i = 0; i < len; i++) {
        Ext num = v.ext_from_u64(1), den = num;
        for (u32 j = 0; j < len; j++) {
            if (j == i) continue;
            num = v.ext_mul(num, v.ext_sub(at, v.ext_from_u64(j)));
            den = v.ext_mul(den, v.ext_sub(v.ext_from_u64(i), v.ext_from_u64(j)));
        }
        Ext w = v.ext_mul(num, v.ext_inv(den));
        v.mul_ext(p_i + (size_t)i * RE, w, t);
        v.add(res, t, res);
    }
    memcpy(out, res, sizeof(res));
}
// The transcript runs over ALL rounds first (the reference's verifier absorbs and samples per round and checks at the end, verifier.rs:56-121); then the
// round checks p(0) + p(1) == expected.  false on a failed check: *failed_round (optional) = its index, expected_out untouched
template <class V>
bool sumcheck_verify(const V &v, typename V::Tr &tr, u32 nv, u32 degree, const u64 *claimed, const u64 *msgs, std::vector<typename V::Ext> &point,
                     u64 *expected_out, u32 *failed_round = nullptr) {
    constexpr int RE = V::RE;
    lfs::sumcheck_prologue<V>(tr, nv, degree);
    point.resize(nv);
    for (u32 i = 0; i < nv; i++) point[i] = lfs::sumcheck_round<V>(tr, msgs + (size_t)i * (degree + 1) * RE, degree + 1);
    u64 expected[RE], s[RE];
    memcpy(expected, claimed, sizeof(expected));
    for (u32 i = 0; i < nv; i++) {
        const u64 *ev = msgs + (size_t)i * (degree + 1) * RE;
        v.add(ev, ev + RE, s);
        if (memcmp(s, expected, sizeof(s))) {
            if (failed_round) *failed_round = i;
            return false;
        }
        interpolate_uni_poly(v, ev, degree + 1, point[i], expected);
    }
    memcpy(expected_out, expected, sizeof(expected));
    return true;
}

// lf_mlsumcheck_verify after its argument checks, for either ring: a word >= p in the claim or the messages -> LF_ERR_INVALID (before the transcript is
// touched); LF_OK with the point (tau words per challenge) and the expected evaluation, or LF_ERR_REJECT with expected_out[0] = the failing round
template <class V>
int mlsumcheck_verify(const V &v, typename V::Tr &tr, u32 nv, u32 degree, const u64 *claimed, const u64 *msgs, u64 *point_out, u64 *expected_out) {
    constexpr int RE = V::RE, TAU = V::TAU;
    for (int w = 0; w < RE; w++)
        if (claimed[w] >= V::modulus()) return LF_ERR_INVALID;
    for (size_t w = 0, nw = (size_t)nv * (degree + 1) * RE; w < nw; w++)
        if (msgs[w] >= V::modulus()) return LF_ERR_INVALID;
    std::vector<typename V::Ext> pt;
    u32 bad = 0;
    const bool ok = sumcheck_verify(v, tr, nv, degree, claimed, msgs, pt, expected_out, &bad);
    for (u32 i = 0; i < nv; i++) {
        u64 rw[RE];
        V::from_ext(pt[i], rw);
        memcpy(point_out + (size_t)i * TAU, rw, TAU * sizeof(u64));
    }
    if (!ok) { memset(expected_out, 0, RE * sizeof(u64)); expected_out[0] = bad; return LF_ERR_REJECT; }
    return LF_OK;
}

template <class V>
struct Verifier {
    typedef typename V::Ext Ext;
    typedef typename V::Tr Tr;
    static constexpr int RE = V::RE, TAU = V::TAU;
    const V &v;
    const lf_params &P;
    const u32 *S_off, *S_idx;
    const u64 *cc;   // q ring elements
    int stage = 0;   // which check rejected

    Verifier(const V &vv, const lf_params &p, const u32 *so, const u32 *si, const u64 *c) : v(vv), P(p), S_off(so), S_idx(si), cc(c) {}

    size_t lcccs_len() const { return (size_t)P.s + TAU + P.kappa + P.t + P.l + 1; }
    size_t cccs_len() const { return (size_t)P.kappa + P.l; }
    size_t lin_len() const { return (size_t)P.s * (P.d + 2) + TAU + P.t; }
    size_t dec_len() const { return (size_t)P.K * (P.t + TAU + P.l + 1 + P.kappa); }

    // eq_eval (utils/sumcheck/utils.rs:78-92) on diagonal points
    Ext eq_eval(const Ext *x, const Ext *y, u32 n) const {
        Ext res = v.ext_from_u64(1), one = res;
        for (u32 i = 0; i < n; i++) {
            Ext xy = v.ext_mul(x[i], y[i]);
            Ext u = v.ext_add(v.ext_sub(v.ext_sub(v.ext_add(xy, xy), x[i]), y[i]), one);
            res = v.ext_mul(res, u);
        }
        return res;
    }
    // verify_as_subprotocol: returns false on a failed round check
    bool sumcheck(Tr &tr, u32 nv, u32 degree, const u64 *claimed, const u64 *msgs, std::vector<Ext> &point, u64 *expected_out) const {
        return sumcheck_verify(v, tr, nv, degree, claimed, msgs, point, expected_out);
    }
    void write_point(const std::vector<Ext> &pt, u64 *o) const {
        for (size_t i = 0; i < pt.size(); i++) v.from_ext(pt[i], o + i * RE);
    }

    bool verify_linearization(Tr &tr, const u64 *cccs, const u64 *proof, u64 *lcccs_out) {
        std::vector<Ext> beta, pt;
        lfs::draw_challenges<V>(tr, "beta_s", P.s, beta);
        u64 zero[RE] = {0}, s[RE];
        if (!sumcheck(tr, P.s, P.d + 1, zero, proof, pt, s)) { stage = 1; return false; }
        const u64 *vv = proof + (size_t)P.s * (P.d + 2) * RE, *u = vv + (size_t)TAU * RE;
        Ext e = eq_eval(pt.data(), beta.data(), P.s);
        u64 sum[RE] = {0}, term[RE];
        for (u32 i = 0; i < P.q; i++) {
            memcpy(term, cc + (size_t)i * RE, sizeof(term));
            for (u32 k = S_off[i]; k < S_off[i + 1]; k++) v.mul(term, u + (size_t)S_idx[k] * RE, term);
            v.add(sum, term, sum);
        }
        v.mul_ext(sum, e, sum);
        if (memcmp(sum, s, sizeof(s))) { stage = 2; return false; }
        tr.absorb_ring(vv, TAU);
        tr.absorb_ring(u, P.t);
        u64 *o = lcccs_out;
        write_point(pt, o); o += (size_t)P.s * RE;
        memcpy(o, vv, (size_t)TAU * RE * 8); o += (size_t)TAU * RE;
        memcpy(o, cccs, (size_t)P.kappa * RE * 8); o += (size_t)P.kappa * RE;
        memcpy(o, u, (size_t)P.t * RE * 8); o += (size_t)P.t * RE;
        memcpy(o, cccs + (size_t)P.kappa * RE, (size_t)P.l * RE * 8); o += (size_t)P.l * RE;
        v.from_u64(1, o);
        return true;
    }
    bool verify_decomposition(Tr &tr, const u64 *lcccs, const u64 *proof, std::vector<u64> &out_K, int stage_id) {
        u32 K = P.K;
        const u64 *u_s = proof, *v_s = u_s + (size_t)K * P.t * RE, *x_s = v_s + (size_t)K * TAU * RE, *y_s = x_s + (size_t)K * (P.l + 1) * RE;
        lfs::absorb_decomposition<V>(tr, P, lcccs, proof, out_K);
        // recomposition checks with b^k (calculate_b_s, recompose_commitment, recompose)
        struct { const u64 *parts; u32 cnt; const u64 *want; } chk[4] = {
            {y_s, P.kappa, lcccs + ((size_t)P.s + TAU) * RE},
            {v_s, (u32)TAU, lcccs + (size_t)P.s * RE},
            {u_s, P.t, lcccs + ((size_t)P.s + TAU + P.kappa) * RE},
            {x_s, P.l + 1, lcccs + ((size_t)P.s + TAU + P.kappa + P.t) * RE},
        };
        for (int c = 0; c < 4; c++)
            for (u32 j = 0; j < chk[c].cnt; j++) {
                u64 a[RE] = {0}, t[RE], bk[RE];
                u64 pw = 1;
                for (u32 k = 0; k < K; k++) {
                    v.from_u64(pw, bk);
                    v.mul(chk[c].parts + ((size_t)k * chk[c].cnt + j) * RE, bk, t);
                    v.add(a, t, a);
                    pw = v.fmul(pw, P.b);
                }
                if (memcmp(a, chk[c].want + (size_t)j * RE, sizeof(a))) { stage = stage_id; return false; }
            }
        return true;
    }

    // returns LF_OK / LF_ERR_REJECT; lcccs_out = folded instance
    // Input validation (untrusted proof bytes): parameter envelope, multiset structure, canonical residues everywhere, diagonal
    // evaluation point.  The arithmetic and the equality checks below assume canonical words; arkworks' deserializer rejects
    // non-canonical field elements the same way (Validate::Yes).
    int validate(const u64 *acc, const u64 *cm_i, const u64 *proof) const {
        if (P.s == 0 || P.s > 40 || P.K == 0 || P.K > 32 || P.q == 0 || P.q > 8 || P.t == 0 || P.t > 16 || P.d == 0 || P.d > 8 ||
            P.b < 2 || P.b > 64 || P.kappa == 0 || P.kappa > 4096 || P.l > 4096 || P.L == 0 || P.L > 64)
            return LF_ERR_UNSUPPORTED;
        if (S_off[0] != 0) return LF_ERR_INVALID;
        for (u32 i = 0; i < P.q; i++)
            if (S_off[i + 1] < S_off[i] || S_off[i + 1] - S_off[i] > P.d) return LF_ERR_INVALID;
        if (S_off[P.q] > 64) return LF_ERR_INVALID;
        for (u32 k = 0; k < S_off[P.q]; k++)
            if (S_idx[k] >= P.t) return LF_ERR_INVALID;
        const u64 p = V::modulus();
        auto canon = [p](const u64 *w, size_t n) {
            for (size_t i = 0; i < n; i++)
                if (w[i] >= p) return false;
            return true;
        };
        const size_t proof_len = lin_len() + 2 * dec_len() + (size_t)P.s * (2 * P.b + 1) + 2 * (size_t)P.K * (TAU + P.t);
        if (!canon(cc, (size_t)P.q * RE) || !canon(acc, lcccs_len() * RE) || !canon(cm_i, cccs_len() * RE) || !canon(proof, proof_len * RE))
            return LF_ERR_INVALID;
        std::vector<Ext> r;   // acc.r: diagonal embeddings of F_{p^tau} challenges
        return lfs::lcccs_point<V>(P, acc, r) ? LF_OK : LF_ERR_UNSUPPORTED;
    }

    int verify(Tr &tr, const u64 *acc, const u64 *cm_i, const u64 *proof, u64 *lcccs_out) {
        int vrc = validate(acc, cm_i, proof);
        if (vrc != LF_OK) return vrc;
        u32 K = P.K, K2 = 2 * K;
        size_t ll = lcccs_len();
        lfs::absorb_public_input<V>(tr, P, acc, cm_i);
        const u64 *lin_proof = proof, *decl = lin_proof + lin_len() * RE, *decr = decl + dec_len() * RE, *foldp = decr + dec_len() * RE;
        std::vector<u64> lin(ll * RE), parts[2];
        auto part = [&](u32 i) { return parts[i / K].data() + (size_t)(i % K) * ll * RE; };   // the 2K decomposed instances
        if (!verify_linearization(tr, cm_i, lin_proof, lin.data())) return LF_ERR_REJECT;
        if (!verify_decomposition(tr, acc, decl, parts[0], 3)) return LF_ERR_REJECT;
        if (!verify_decomposition(tr, lin.data(), decr, parts[1], 4)) return LF_ERR_REJECT;

        // LFFoldingVerifier::verify
        std::vector<Ext> alpha, zeta, mu, beta, r0;
        lfs::draw_alpha_zeta<V>(tr, K2, alpha, zeta);
        lfs::draw_mu_beta<V>(tr, K2, P.s, mu, beta);
        // calculate_claims: sum_i sum_j alpha_i^{j+1} v_ij + zeta_i^{j+1} u_ij
        u64 claim[RE] = {0}, t[RE];
        for (u32 i = 0; i < K2; i++) {
            const u64 *li = part(i);
            lfs::powers(v, alpha[i], TAU, [&](u32 d, const Ext &pw) { v.mul_ext(li + ((size_t)P.s + d) * RE, pw, t); v.add(claim, t, claim); });
            lfs::powers(v, zeta[i], P.t, [&](u32 j, const Ext &pw) { v.mul_ext(li + ((size_t)P.s + TAU + P.kappa + j) * RE, pw, t); v.add(claim, t, claim); });
        }
        u64 expected[RE];
        u32 deg = 2 * P.b;
        if (!sumcheck(tr, P.s, deg, claim, foldp, r0, expected)) { stage = 5; return LF_ERR_REJECT; }
        const u64 *theta = foldp + (size_t)P.s * (deg + 1) * RE, *eta = theta + (size_t)K2 * TAU * RE;
        {   // verify_evaluation / compute_sumcheck_claim_expected_value
            Ext e_ast = eq_eval(beta.data(), r0.data(), P.s);
            u64 total[RE] = {0}, s1[RE], s2[RE], s3[RE], th2[RE], prod[RE], bb[RE], m2[RE];
            std::vector<Ext> ri;
            for (u32 i = 0; i < K2; i++) {
                if (!lfs::lcccs_point<V>(P, part(i), ri)) return LF_ERR_UNSUPPORTED;   // (acc.r was validated, the other point was written by write_point)
                Ext e_i = eq_eval(ri.data(), r0.data(), P.s);
                memset(s1, 0, sizeof(s1)); memset(s2, 0, sizeof(s2)); memset(s3, 0, sizeof(s3));
                lfs::powers(v, alpha[i], TAU, [&](u32 d, const Ext &pw) { v.mul_ext(theta + ((size_t)i * TAU + d) * RE, v.ext_mul(pw, e_i), t); v.add(s1, t, s1); });
                lfs::powers(v, mu[i], TAU, [&](u32 d, const Ext &pw) {
                    const u64 *th = theta + ((size_t)i * TAU + d) * RE;
                    v.mul(th, th, th2);
                    v.from_u64(1, prod);
                    for (u32 b = 1; b < P.b; b++) { v.from_u64((u64)b * b, bb); v.sub(th2, bb, m2); v.mul(prod, m2, prod); }
                    v.mul(th, prod, t); v.mul_ext(t, pw, t); v.add(s2, t, s2);
                });
                v.mul_ext(s2, e_ast, s2);
                lfs::powers(v, zeta[i], P.t, [&](u32 j, const Ext &pw) { v.mul_ext(eta + ((size_t)i * P.t + j) * RE, pw, t); v.add(s3, t, s3); });
                v.mul_ext(s3, e_i, s3);
                v.add(total, s1, total); v.add(total, s2, total); v.add(total, s3, total);
            }
            if (memcmp(total, expected, sizeof(total))) { stage = 6; return LF_ERR_REJECT; }
        }
        tr.absorb_ring(theta, (size_t)K2 * TAU);
        tr.absorb_ring(eta, (size_t)K2 * P.t);
        std::vector<u64> rho_c, rho;
        lfs::draw_rho(v, tr, K2, rho_c, rho);
        lfs::fold_instance(v, P, r0, theta, eta, rho_c.data(), rho.data(), part, lcccs_out);
        return LF_OK;
    }
};

}  // namespace lfv
