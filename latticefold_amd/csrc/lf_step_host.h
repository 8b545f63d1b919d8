// lf_step_host.h -- the host arithmetic of one fold step (NIFSProver::prove / NIFSVerifier::verify, crates/latticefold/src/nifs.rs:48-163), ONCE for both rings
// and for both sides of the protocol: the transcript steps and the instance arithmetic that the Goldilocks prover (lf_prove.cpp, lf_fold.cpp, lf_fold_sb.cpp),
// the BabyBear prover (bb_prove.cpp) and the verifier (lf_verify.h) have in common.  Host only: no HIP header, no launcher, plain C++17.
//
// `V` is the ring's host policy (GoldV in lf_host.h, BbV in bb_host.h): a plain struct of small inline functions that REFERS to a host ring -- the context's in
// the provers (a context may carry other tables than the default ring), the default one in lf_verify_host.  Functions that need the tables take `v`; the
// others name the policy (`lfs::sumcheck_round<GoldV>(tr, ..)`).
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
