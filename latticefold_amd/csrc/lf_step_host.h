// lf_step_host.h -- the host arithmetic of one fold step (NIFSProver::prove / NIFSVerifier::verify, crates/latticefold/src/nifs.rs:48-163), ONCE for both rings
// and for both sides of the protocol: the transcript steps and the instance arithmetic that the Goldilocks prover (lf_prove.cpp, lf_fold.cpp, lf_fold_sb.cpp),
// the BabyBear prover (bb_prove.cpp) and the verifier (lf_verify.h) have in common.  Host only: no HIP header, no launcher, plain C++17.
//
// `V` is the ring's host policy (GoldV in lf_host.h, BbV in bb_host.h): a plain struct of small inline functions that REFERS to a host ring -- the context's in
// the provers (a context may carry other tables than the default ring), the default one in lf_verify_host.  Functions that need the tables take `v`; the
// others name the policy (`lfs::sumcheck_round<GoldV>(tr, ..)`).  The numeric host work inside the sumcheck rounds of the provers is here too: eq weights, the
// digit look-up table, the completion of a split round message and its invertibility test.
//
// What belongs to a prover's schedule stays at its call sites: the HostTimer scopes and the host_tr_ms accounting, the timeline marks, the waits and
// downloads in front of a call.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/lfhip.h"

namespace lfs {

typedef uint64_t u64;
typedef uint32_t u32;

// ---- sumcheck transcript (utils/sumcheck.rs:60-62 and the round step of prove_as_subprotocol / verify_as_subprotocol) -------------------------------
template <class V>
void sumcheck_prologue(typename V::Tr &tr, u32 nv, u32 deg) {
    tr.absorb_u64_as_ring(nv);
    tr.absorb_u64_as_ring(deg);
}
// absorb the round message, draw the challenge, absorb it
template <class V>
typename V::Ext sumcheck_round(typename V::Tr &tr, const u64 *evals, u32 npts) {
    tr.absorb_ring(evals, npts);
    typename V::Ext r = tr.get_challenge();
    V::absorb_ext(tr, r);
    return r;
}

// the LCCCS point r as extension-field challenges; false if an element is not a diagonal embedding
template <class V>
bool lcccs_point(const lf_params &P, const u64 *lcccs, std::vector<typename V::Ext> &pt) {
    pt.resize(P.s);
    for (u32 i = 0; i < P.s; i++)
        if (!V::is_diag(lcccs + (size_t)i * V::RE, &pt[i])) return false;
    return true;
}

// absorb_public_input (nifs.rs:175-197)
template <class V>
void absorb_public_input(typename V::Tr &tr, const lf_params &P, const u64 *acc, const u64 *cm_i) {
    tr.absorb_label("acc");
    tr.absorb_ring(acc, (size_t)P.s + V::TAU + P.kappa + P.t + P.l + 1);
    tr.absorb_label("cm_i");
    tr.absorb_ring(cm_i, (size_t)P.kappa + P.l);
}

// ---- decomposition (nifs/decomposition.rs:33-88) ------------------------------------------------------------------------------------------------------
// decompose_big_vec_into_k_vec_and_compose_back (nifs/decomposition/utils.rs:12-42) on the l + 1 elements xh (NTT form) -> x_s [K][l + 1]
template <class V>
void decompose_x(const V &v, const lf_params &P, int digit_mode, const u64 *xh, u64 *x_s) {
    constexpr int RE = V::RE;
    const u32 cnt = P.l + 1;
    u64 co[RE];
    std::vector<int64_t> dB(P.L), dk(P.K);
    std::vector<u64> part((size_t)P.K * RE);
    for (u32 i = 0; i < cnt; i++) {
        v.icrt(xh + (size_t)i * RE, co);
        std::fill(part.begin(), part.end(), 0);
        for (int cc = 0; cc < RE; cc++) {   // per coefficient: L digits base B, each K digits base b
            V::balanced_digits(co[cc], P.B, P.L, dB.data(), digit_mode);
            u64 pw = 1;
            for (u32 l = 0; l < P.L; l++) {
                V::balanced_digits(V::from_i64(dB[l]), P.b, P.K, dk.data(), digit_mode);
                for (u32 k = 0; k < P.K; k++) part[(size_t)k * RE + cc] = V::fadd(part[(size_t)k * RE + cc], V::fmul(pw, V::from_i64(dk[k])));
                pw = V::fmul(pw, P.B);
            }
        }
        for (u32 k = 0; k < P.K; k++) v.crt(&part[(size_t)k * RE], x_s + ((size_t)k * cnt + i) * RE);
    }
}

// y_0 = cm - sum_{k>=1} b^k y_k, as the reference's fold (acc + y_i) * b.  y_s: [K][kappa] elements, parts 1 .. K-1 in (words reduced mod p here), part 0 out.
// (b is a base-field constant: in the NTT form the product with it is the word-wise one -- RE multiplications per element instead of eight extension products)
template <class V>
void commit_y0(const lf_params &P, const u64 *cm, u64 *y_s) {
    constexpr int RE = V::RE;
    std::vector<u64> acc((size_t)P.kappa * RE, 0);
    for (int k = (int)P.K - 1; k >= 1; k--)
        for (size_t w = 0; w < acc.size(); w++) acc[w] = V::fmul(V::fadd(acc[w], y_s[(size_t)k * P.kappa * RE + w] % V::modulus()), P.b);
    for (u32 i = 0; i < P.kappa; i++) V::sub(cm + (size_t)i * RE, &acc[(size_t)i * RE], y_s + (size_t)i * RE);
}

// transcript part of the decomposition (decomposition.rs:65-83): absorb x_k, y_k, u_k, v_k of the K parts and assemble their LCCCS into `out` ([K] flat
// LCCCS).  No challenge is drawn here.
template <class V>
void absorb_decomposition(typename V::Tr &tr, const lf_params &P, const u64 *lcccs, const u64 *proof, std::vector<u64> &out) {
    constexpr size_t RE = V::RE, TAU = V::TAU;
    const u32 K = P.K;
    const u64 *u_s = proof, *v_s = u_s + (size_t)K * P.t * RE, *x_s = v_s + (size_t)K * TAU * RE, *y_s = x_s + (size_t)K * (P.l + 1) * RE;
    const size_t ll = (size_t)P.s + TAU + P.kappa + P.t + P.l + 1;
    out.assign((size_t)K * ll * RE, 0);
    for (u32 k = 0; k < K; k++) {
        const u64 *xk = x_s + (size_t)k * (P.l + 1) * RE, *yk = y_s + (size_t)k * P.kappa * RE;
        const u64 *uk = u_s + (size_t)k * P.t * RE, *vk = v_s + (size_t)k * TAU * RE;
        tr.absorb_ring(xk, P.l + 1);
        tr.absorb_ring(yk, P.kappa);
        tr.absorb_ring(uk, P.t);
        tr.absorb_ring(vk, TAU);
        u64 *o = &out[(size_t)k * ll * RE];
        memcpy(o, lcccs, (size_t)P.s * RE * 8); o += (size_t)P.s * RE;
        memcpy(o, vk, TAU * RE * 8); o += TAU * RE;
        memcpy(o, yk, (size_t)P.kappa * RE * 8); o += (size_t)P.kappa * RE;
        memcpy(o, uk, (size_t)P.t * RE * 8); o += (size_t)P.t * RE;
        memcpy(o, xk, (size_t)(P.l + 1) * RE * 8);
    }
}

// ---- folding (nifs/folding.rs:42-195) -----------------------------------------------------------------------------------------------------------------
// The challenges of folding/utils.rs:52-95 in transcript order alpha, zeta, mu, beta -- in two calls, because both provers queue GPU work that needs alpha
// and zeta only between them.
template <class V>
void draw_challenges(typename V::Tr &tr, const char *label, size_t n, std::vector<typename V::Ext> &out) {
    tr.absorb_label(label);
    out.resize(n);
    for (size_t i = 0; i < n; i++) out[i] = tr.get_challenge();
}
template <class V>
void draw_alpha_zeta(typename V::Tr &tr, u32 K2, std::vector<typename V::Ext> &alpha, std::vector<typename V::Ext> &zeta) {
    draw_challenges<V>(tr, "alpha_s", K2, alpha);
    draw_challenges<V>(tr, "zeta_s", K2, zeta);
}
template <class V>
void draw_mu_beta(typename V::Tr &tr, u32 K2, u32 s, std::vector<typename V::Ext> &mu, std::vector<typename V::Ext> &beta) {
    draw_challenges<V>(tr, "mu_s", K2 - 1, mu);
    mu.push_back(V::ext_from_u64(1));   // the constant ONE comes last (folding/utils.rs:83)
    draw_challenges<V>(tr, "beta_s", s, beta);
}
// fn(j, x^{j+1}) for j < n
template <class V, class Fn>
void powers(const V &v, const typename V::Ext &x, u32 n, Fn fn) {
    typename V::Ext p = x;
    for (u32 j = 0; j < n; j++) {
        fn(j, p);
        p = v.ext_mul(p, x);
    }
}

// get_rhos (folding/utils.rs:116-131): the 2K short challenges (ONE last) in coefficient form rho_c [K2][RE], NTT form rho [K2][RE] and, if asked for, as
// centred int8 coefficients rho8 [K2][RHO8] -- the layout launch_fold_witness takes (a short challenge has its non-zero coefficients below RHO8 on both rings)
constexpr int RHO8 = 24;
template <class V>
void draw_rho(const V &v, typename V::Tr &tr, u32 K2, std::vector<u64> &rho_c, std::vector<u64> &rho, std::vector<int8_t> *rho8 = nullptr) {
    constexpr size_t RE = V::RE;
    rho_c.assign((size_t)K2 * RE, 0);
    rho.assign((size_t)K2 * RE, 0);
    tr.absorb_label("rho_s");
    for (u32 i = 0; i + 1 < K2; i++) tr.get_short_challenge(&rho_c[(size_t)i * RE]);
    rho_c[(size_t)(K2 - 1) * RE] = 1;
    for (u32 i = 0; i < K2; i++) v.crt(&rho_c[(size_t)i * RE], &rho[(size_t)i * RE]);
    if (!rho8) return;
    rho8->assign((size_t)K2 * RHO8, 0);
    const u64 p = V::modulus();
    for (u32 i = 0; i < K2; i++)
        for (int q = 0; q < RHO8; q++) {
            const u64 c = rho_c[(size_t)i * RE + q];
            (*rho8)[(size_t)i * RHO8 + q] = (int8_t)(c > p / 2 ? -(int64_t)(p - c) : (int64_t)c);
        }
}

// v_0 = rot_lin_combination(rho_coeff, theta) (cyclotomic-rings/src/rotation.rs:85-104) -> out, TAU elements: sum_i rho_i(X) Theta_i(X) modulo the cyclotomic
// polynomial, where Theta_i(X) = sum_b theta_i[b] X^b has the TAU-word groups of the TAU elements theta_i as coefficients.  As one polynomial product per i --
// full[a + b] += rho_a theta_b over the non-zero coefficients of rho and all of theta: the inner loop is one contiguous multiply-add over theta's RE x TAU
// words -- and ONE reduction of the degree-(2 RE - 2) product by X^RE = X^(RE/2) - 1 at the end.  (The rotation-by-rotation form walks RE x RE pairs per i
// with rotations that fill up.)  The arithmetic is exact in either form; how a term is accumulated is the policy's (V::Acc).
template <class V>
void fold_v0(u32 K2, const u64 *theta, const u64 *rho_c, u64 *out) {
    constexpr int RE = V::RE, TAU = V::TAU;
    typedef typename V::Acc Acc;
    std::vector<Acc> acc((size_t)(2 * RE) * TAU, Acc(0));
    for (u32 i = 0; i < K2; i++)
        for (int a = 0; a < RE; a++) {
            const Acc r = V::acc_coef(rho_c[(size_t)i * RE + a]);
            if (r != Acc(0)) V::acc_mac(&acc[(size_t)a * TAU], theta + (size_t)i * TAU * RE, RE * TAU, r);
        }
    for (int d = 2 * RE - 2; d >= RE; d--)
        for (int q = 0; q < TAU; q++) V::acc_fold(acc[(size_t)(d - RE / 2) * TAU + q], acc[(size_t)(d - RE) * TAU + q], acc[(size_t)d * TAU + q]);
    for (int x = 0; x < RE * TAU; x++) out[x] = V::acc_word(acc[x]);
}

// compute_v0_u0_x0_cm_0 (folding/utils.rs:460-521): the folded LCCCS from the point, theta, eta, the challenges rho_i and the 2K decomposed instances
// (part(i) = the i-th of them, flat).
template <class V, class PartFn>
void fold_instance(const V &v, const lf_params &P, const std::vector<typename V::Ext> &pt, const u64 *theta, const u64 *eta, const u64 *rho_c, const u64 *rho,
                   PartFn part, u64 *lcccs_out) {
    constexpr int RE = V::RE, TAU = V::TAU;
    const u32 K2 = 2 * P.K;
    u64 *o = lcccs_out;
    for (u32 i = 0; i < P.s; i++, o += RE) V::from_ext(pt[i], o);
    fold_v0<V>(K2, theta, rho_c, o);
    o += (size_t)TAU * RE;
    u64 tmp[RE];
    const size_t cm = (size_t)P.s + TAU, u = cm + P.kappa, x = u + P.t;   // offsets in an LCCCS (elements)
    for (u32 c = 0; c < P.kappa; c++, o += RE) {
        memset(o, 0, RE * 8);
        for (u32 i = 0; i < K2; i++) { v.mul(part(i) + (cm + c) * RE, rho + (size_t)i * RE, tmp); V::add(o, tmp, o); }
    }
    for (u32 j = 0; j < P.t; j++, o += RE) {
        memset(o, 0, RE * 8);
        for (u32 i = 0; i < K2; i++) { v.mul(rho + (size_t)i * RE, eta + ((size_t)i * P.t + j) * RE, tmp); V::add(o, tmp, o); }
    }
    for (u32 c = 0; c < P.l + 1; c++, o += RE) {
        memset(o, 0, RE * 8);
        for (u32 i = 0; i < K2; i++) { v.mul(rho + (size_t)i * RE, part(i) + (x + c) * RE, tmp); V::add(o, tmp, o); }
    }
}

// ---- the numeric host work inside the sumcheck rounds: eq weights, the digit look-up table, the completion of a split message -------------------------
// An Ext of either ring is TAU canonical words `c`; a message is [X][RE] words with slot k at word TAU k.
template <class V>
bool ext_is_zero(const typename V::Ext &x) { return std::all_of(x.c, x.c + V::TAU, [](u64 w) { return w == 0; }); }
template <class V>
typename V::Ext ext_load(const u64 *w) {
    typename V::Ext r;
    for (int i = 0; i < V::TAU; i++) r.c[i] = w[i] % V::modulus();
    return r;
}
template <class V>
typename V::Ext eq1(const V &v, const typename V::Ext &b, const typename V::Ext &r) {   // eq(b, r) = (1 - b)(1 - r) + b r
    const typename V::Ext one = V::ext_from_u64(1);
    return V::ext_add(v.ext_mul(V::ext_sub(one, b), V::ext_sub(one, r)), v.ext_mul(b, r));
}
// W_b = eq((r_1..r_nbits), b) for the 2^nbits indices b, LSB-first (bit j of b goes with r_{j+1} = pt[j])
template <class V>
void eq_weights(const V &v, const typename V::Ext *pt, u32 nbits, typename V::Ext *W) {
    const typename V::Ext one = V::ext_from_u64(1);
    for (u32 b = 0; b < (1u << nbits); b++) {
        W[b] = one;
        for (u32 j = 0; j < nbits; j++) W[b] = v.ext_mul(W[b], ((b >> j) & 1) ? pt[j] : V::ext_sub(one, pt[j]));
    }
}
// c_round = prod_{k < round} eq(beta_k, r_k) (rounds count from 1: beta_k = beta[k - 1], r_k = pt[k - 1])
template <class V>
typename V::Ext eq_prefix(const V &v, const typename V::Ext *beta, const typename V::Ext *pt, u32 round) {
    typename V::Ext c = V::ext_from_u64(1);
    for (u32 k = 1; k < round; k++) c = v.ext_mul(c, eq1(v, beta[k - 1], pt[k - 1]));
    return c;
}
// Lagrange weights of the nodes 0..deg at x: p(x) = sum_j w[j] p(j) for a polynomial of degree <= deg
template <class V>
void lagrange_weights(const V &v, u32 deg, const typename V::Ext &x, typename V::Ext *w) {
    for (u32 j = 0; j <= deg; j++) {
        typename V::Ext num = V::ext_from_u64(1);
        u64 den = 1;
        for (u32 k = 0; k <= deg; k++) {
            if (k == j) continue;
            num = v.ext_mul(num, V::ext_sub(x, V::ext_from_u64(k)));
            den = V::fmul(den, V::from_i64((int64_t)j - (int64_t)k));
        }
        w[j] = V::ext_scale(num, V::finv(den));
    }
}
// lut[code] = sum_b (t_b - 1) W_b for the 81 codes sum_b t_b 3^b of four ternary digits, W_b = eq((r1, r2), b); out[81 + code] = its square
template <class V>
void fold_lut81(const V &v, const typename V::Ext &r1, const typename V::Ext &r2, typename V::Ext *out /* [162] */) {
    const typename V::Ext pt[2] = {r1, r2};
    typename V::Ext W[4];
    eq_weights(v, pt, 2, W);
    for (int code = 0; code < 81; code++) {
        typename V::Ext x = V::ext_from_u64(0);
        int cc = code;
        for (int b = 0; b < 4; b++, cc /= 3) {
            if (cc % 3 == 2) x = V::ext_add(x, W[b]);
            else if (cc % 3 == 0) x = V::ext_sub(x, W[b]);
        }
        out[code] = x;
        out[81 + code] = v.ext_mul(x, x);
    }
}
// The split form of a round: the kernel sums against E_i[p] only, and the host completes g_i(X) = c_i eq(beta_i, X) T_i(X) (+ G(X)).  The value the kernel
// leaves out follows from g_i(0) + g_i(1) = g_{i-1}(r_{i-1}) -- which divides by c_i and beta_i: `ok` is the one test of both completions (a driver that
// finds it false runs the round unsplit).
template <class V>
struct SplitCoef {
    typename V::Ext c, bi, cinv, binv;
    bool ok;
};
template <class V>
SplitCoef<V> split_coef(const V &v, const typename V::Ext &c, const typename V::Ext &bi) {
    SplitCoef<V> s{c, bi, V::ext_from_u64(0), V::ext_from_u64(0), false};
    if (ext_is_zero<V>(c) || ext_is_zero<V>(bi)) return s;
    s.cinv = v.ext_inv(c);
    s.binv = v.ext_inv(bi);
    s.ok = !ext_is_zero<V>(s.cinv) && !ext_is_zero<V>(s.binv);
    return s;
}
// shared tail of both completions: T(1) (slot-wise) from the previous message `prev` ([deg + 1][RE]) at its challenge x, less gsum = G(0) + G(1) if any
template <class V>
typename V::Ext split_T1(const V &v, const SplitCoef<V> &s, const typename V::Ext *wS, u32 deg, const u64 *prev, u32 slot, const typename V::Ext &T0,
                         const typename V::Ext *gsum) {
    typename V::Ext S = V::ext_from_u64(0);
    for (u32 j = 0; j <= deg; j++) S = V::ext_add(S, v.ext_mul(wS[j], ext_load<V>(prev + (size_t)j * V::RE + V::TAU * slot)));
    if (gsum) S = V::ext_sub(S, *gsum);
    // c (l(0) T(0) + l(1) T(1)) = S,  l(0) = 1 - beta_i, l(1) = beta_i
    return v.ext_mul(V::ext_sub(v.ext_mul(S, s.cinv), v.ext_mul(V::ext_sub(V::ext_from_u64(1), s.bi), T0)), s.binv);
}
template <class V>
void split_store(const V &v, const SplitCoef<V> &s, u32 deg, const typename V::Ext *T, const u64 *G, u32 slot, u64 *out) {
    const typename V::Ext obi = V::ext_sub(V::ext_from_u64(1), s.bi), dl = V::ext_sub(s.bi, obi);
    typename V::Ext l = obi;   // eq(beta_i, X) = (1 - beta_i) + X (2 beta_i - 1)
    for (u32 X = 0; X <= deg; X++) {
        typename V::Ext g = v.ext_mul(v.ext_mul(s.c, l), T[X]);
        if (G) g = V::ext_add(g, ext_load<V>(G + (size_t)X * V::RE + V::TAU * slot));
        memcpy(out + (size_t)X * V::RE + V::TAU * slot, g.c, sizeof(g.c));
        l = V::ext_add(l, dl);
    }
}
// Folding sumcheck (degree 4): A [3][RE] = the sums A_e = sum_p E[p] Q_e(p), G [5][RE] = the G part eqL G1 + eqR G2 at X = 0..4, prev = the previous
// message, x its challenge.  g(X) = c l(X) (A0 + A1 X + A2 X^2 + A3 X^3) + G(X), A3 from g(0) + g(1) = prev(x).  out [5][RE].
template <class V>
void complete_fold_split(const V &v, const SplitCoef<V> &s, const u64 *A, const u64 *G, const u64 *prev, const typename V::Ext &x, u64 *out) {
    typedef typename V::Ext Ext;
    constexpr u32 deg = 4;
    Ext wS[deg + 1];
    lagrange_weights(v, deg, x, wS);
    for (u32 slot = 0; slot < 8; slot++) {
        auto ld = [&](const u64 *b, u32 e) { return ext_load<V>(b + (size_t)e * V::RE + V::TAU * slot); };
        const Ext A0 = ld(A, 0), A1 = ld(A, 1), A2 = ld(A, 2), gsum = V::ext_add(ld(G, 0), ld(G, 1));
        const Ext T1 = split_T1(v, s, wS, deg, prev, slot, A0, &gsum);   // T(1) = A0 + A1 + A2 + A3
        const Ext A3 = V::ext_sub(V::ext_sub(V::ext_sub(T1, A0), A1), A2);
        Ext T[deg + 1];
        for (u32 X = 0; X <= deg; X++) T[X] = V::ext_add(A0, V::ext_scale(V::ext_add(A1, V::ext_scale(V::ext_add(A2, V::ext_scale(A3, X)), X)), X));
        split_store(v, s, deg, T, G, slot, out);
    }
}
// Linearization sumcheck: Tv [dT + 1][RE] = T(X) = sum_p E[p] h(X, p) at X = 0..dT -- all of them in round 1 (prev = nullptr), X = 1 missing afterwards (from
// prev, the previous message of degree dT + 1, at its challenge x).  T has degree dT <= 7: its value at dT + 1 from the vanishing (dT+1)-th finite
// difference.  out [dT + 2][RE] = g(X) = c eq(beta_i, X) T(X).
template <class V>
void complete_lin_split(const V &v, const SplitCoef<V> &s, u32 dT, const u64 *Tv, const u64 *prev, const typename V::Ext &x, u64 *out) {
    typedef typename V::Ext Ext;
    static const int binom[9][9] = {{1}, {1, 1}, {1, 2, 1}, {1, 3, 3, 1}, {1, 4, 6, 4, 1}, {1, 5, 10, 10, 5, 1}, {1, 6, 15, 20, 15, 6, 1}, {1, 7, 21, 35, 35, 21, 7, 1},
                                    {1, 8, 28, 56, 70, 56, 28, 8, 1}};
    const u32 deg = dT + 1;
    Ext wS[9];
    if (prev) lagrange_weights(v, deg, x, wS);
    for (u32 slot = 0; slot < 8; slot++) {
        Ext T[9];
        for (u32 X = 0; X <= dT; X++) T[X] = ext_load<V>(Tv + (size_t)X * V::RE + V::TAU * slot);
        if (prev) T[1] = split_T1(v, s, wS, deg, prev, slot, T[0], nullptr);
        Ext top = V::ext_from_u64(0);
        for (u32 j = 0; j <= dT; j++) {
            const Ext term = V::ext_scale(T[j], (u64)binom[dT + 1][j]);
            top = ((dT - j) & 1) ? V::ext_sub(top, term) : V::ext_add(top, term);
        }
        T[dT + 1] = top;
        split_store(v, s, deg, T, nullptr, slot, out);
    }
}

// C_pi(X) of lf_sv_rounds.h for the nV weights W_b = eq((r_1..), b): the coefficient table [npairs][4] of the GEMM rounds.  h = sum_x w_x(X) y_x with
// w_x = W_x (1 - X) (x < nV), W_{x-nV} X (x >= nV); h^3 - h expanded over y^2 = b, y^3 = y.  pair(i) = the i-th (sign subset, bit subset) of the canonical
// order (sv_pair); each caller packs the table into its word form.
template <class V, class PairFn>
void sv_coef(const V &v, int nV, const typename V::Ext *W, int npairs, PairFn pair, std::vector<typename V::Ext> &C) {
    typedef typename V::Ext Ext;
    const int NX = 2 * nV;
    const Ext zero = V::ext_from_u64(0);
    C.assign((size_t)npairs * 4, zero);
    std::vector<decltype(pair(0))> prs(npairs);
    for (int i = 0; i < npairs; i++) prs[i] = pair(i);
    auto find = [&](unsigned s, unsigned b) {
        for (int i = 0; i < npairs; i++)
            if (prs[i].s == s && prs[i].b == b) return i;
        return -1;
    };
    // w_x(X) = wa_x + wb_x X
    std::vector<Ext> wa(NX), wb(NX);
    for (int x = 0; x < NX; x++) {
        if (x < nV) { wa[x] = W[x]; wb[x] = V::ext_sub(zero, W[x]); }
        else { wa[x] = zero; wb[x] = W[x - nV]; }
    }
    // h^3: multisets {x <= y <= z} with their multinomial multiplicity
    for (int x = 0; x < NX; x++)
        for (int y = x; y < NX; y++) {
            const Ext p2[3] = {v.ext_mul(wa[x], wa[y]), V::ext_add(v.ext_mul(wa[x], wb[y]), v.ext_mul(wb[x], wa[y])), v.ext_mul(wb[x], wb[y])};
            for (int z = y; z < NX; z++) {
                const Ext p3[4] = {v.ext_mul(p2[0], wa[z]), V::ext_add(v.ext_mul(p2[0], wb[z]), v.ext_mul(p2[1], wa[z])),
                                   V::ext_add(v.ext_mul(p2[1], wb[z]), v.ext_mul(p2[2], wa[z])), v.ext_mul(p2[2], wb[z])};
                int mult, idx;
                if (x == y && y == z) { mult = 1; idx = find(1u << x, 1u << x); }
                else if (x == y) { mult = 3; idx = find(1u << z, (1u << x) | (1u << z)); }      // y_x^2 y_z = b_x y_z
                else if (y == z) { mult = 3; idx = find(1u << x, (1u << x) | (1u << y)); }      // y_x y_y^2 = y_x b_y
                else { mult = 6; const unsigned mk = (1u << x) | (1u << y) | (1u << z); idx = find(mk, mk); }
                for (int e = 0; e < 4; e++)
                    for (int i = 0; i < mult; i++) C[(size_t)idx * 4 + e] = V::ext_add(C[(size_t)idx * 4 + e], p3[e]);
            }
        }
    for (int x = 0; x < NX; x++) {   // - h
        const int idx = find(1u << x, 1u << x);
        C[(size_t)idx * 4] = V::ext_sub(C[(size_t)idx * 4], wa[x]);
        C[(size_t)idx * 4 + 1] = V::ext_sub(C[(size_t)idx * 4 + 1], wb[x]);
    }
}

}  // namespace lfs
