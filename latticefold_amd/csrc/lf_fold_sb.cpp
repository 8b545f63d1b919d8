// lf_fold_sb.cpp -- the folding prover (nifs/folding.rs:74-179) on the small-base path, b = 4, 8, 16 (lf_sb.h): the sumcheck of nifs/folding/utils.rs:273-325 at
// degree 2b over the norm polynomial f prod_{j=1}^{b-1} (f^2 - j^2), theta / eta, and the fold of the witnesses from their digit planes.  One lane, ordinary
// launches, one host hop per round: round 1 reads the digit planes (f-hat virtual), r_1 materialises the m/2-entry tables, later rounds fix them ping-pong.
#include "lf_ring_host.h"


// One round message from its two device halves: `norm` [X][24] at X = 0 .. 2b (launch_sb_round) and `g` [X][24] at X = 0 .. 4 (launch_fold_round_g).  The G
// part eqL G1 + eqR G2 has degree 2: its values at X >= 3 follow from those at 0, 1, 2 by the vanishing third difference -- exact field arithmetic, the words
// of the reference's message.
static void sb_compose_message(const u64 *norm, const u64 *g, u32 deg, u64 *evs) {
    for (u32 w = 0; w < 24; w++) {
        u64 g0 = g[w], g1 = g[24 + w], g2 = g[48 + w];
        evs[w] = fq_add(norm[w], g0);
        evs[24 + w] = fq_add(norm[24 + w], g1);
        evs[48 + w] = fq_add(norm[48 + w], g2);
        for (u32 X = 3; X <= deg; X++) {   // g(X) = 3 g(X-1) - 3 g(X-2) + g(X-3)
            const u64 d = fq_sub(g2, g1), g3 = fq_add(fq_add(fq_add(d, d), d), g0);
            evs[(size_t)X * 24 + w] = fq_add(norm[(size_t)X * 24 + w], g3);
            g0 = g1; g1 = g2; g2 = g3;
        }
    }
}

// the round of lf_sumcheck_fold_round on uploaded tables: t5 = the 57 special planes (eqL eqR eqB G1 G2, n entries), F = f-hat tables [2K*3][24][n]
int sb_fold_round_abi(lf_ctx *c, const u64 *t5, const u64 *F, size_t n, const Fq3Const *d_mu, u64 *evals_out) {
    const lf_params &P = c->P;
    const u32 deg = 2 * P.b;
    FoldRoundArgs a;
    a.eqL = t5; a.eqR = t5 + 3 * n; a.eqB = t5 + 6 * n; a.G1 = t5 + 9 * n; a.G2 = t5 + 33 * n;
    a.ld = n; a.n = n; a.p0 = 0; a.pcnt = n / 2; a.pF0 = 0;
    u64 *partial, *partial_g, *od;
    RET(c->tbuf("sb_round_partial", sb_round_partial_words(), &partial));
    RET(c->tbuf("round_partial", round_partial_words(), &partial_g));
    RET(c->tbuf("sb_round_out", sb_round_out_words() + 5 * 24, &od));
    if (launch_sb_round(c->dcrt, P.b, a, F, n, nullptr, nullptr, 0, 0, P.K, d_mu, partial, od, c->stream()) != 0) return LF_ERR_HIP;
    launch_fold_round_g(c->dcrt, a, partial_g, od + sb_round_out_words(), c->stream());
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    std::vector<u64> h(sb_round_out_words() + 5 * 24);
    RET(down_small(c, od, h.size(), h.data()));
    sb_compose_message(h.data(), h.data() + sb_round_out_words(), deg, evals_out);
    return LF_OK;
}

int fold_impl_sb(lf_ctx *c, Transcript &tr, SideState *S /* [2] */, u64 *lcccs_out, lf_witness **w_out, u64 *proof) {
    const lf_params &P = c->P;
    const size_t m = c->m, n = c->n, N = c->N, ldn = sb_ld(N);
    const u32 K = P.K, K2 = 2 * K, deg = 2 * P.b;
    if (!sb_base_ok(P.b) || c->sh_world > 1 || !S[0].D || !S[1].D) return LF_ERR_UNSUPPORTED;
    const GoldV hv{c->ring};
    std::vector<Fq3> alpha, zeta, mu, beta;
    {
        HostTimer ht(c);
        lfs::draw_alpha_zeta<GoldV>(tr, K2, alpha, zeta);
        lfs::draw_mu_beta<GoldV>(tr, K2, P.s, mu, beta);
    }
    size_t ph = c->ev_begin(13);
    std::vector<Fq3Const> mu_pow((size_t)K2 * 3), a_pow((size_t)K2 * 3), z_pow((size_t)K2 * P.t);
    for (u32 i = 0; i < K2; i++) {
        lfs::powers(hv, alpha[i], 3, [&](u32 d, const Fq3 &pw) { a_pow[(size_t)i * 3 + d] = f3c(pw); });
        lfs::powers(hv, mu[i], 3, [&](u32 d, const Fq3 &pw) { mu_pow[(size_t)i * 3 + d] = f3c(pw); });
        lfs::powers(hv, zeta[i], P.t, [&](u32 j, const Fq3 &pw) { z_pow[(size_t)i * P.t + j] = f3c(pw); });
    }
    Fq3Const *d_mu, *d_ap, *d_zp;
    RET(upload_consts(c, "c_ap", a_pow, &d_ap));
    RET(upload_consts(c, "c_zp", z_pow, &d_zp));
    RET(upload_consts(c, "c_mu", mu_pow, &d_mu));
    u64 *G[2], *eqb, *zz, *partial, *partial_g, *od;
    RET(c->tbuf("fold_G1", 24 * m, &G[0]));
    RET(c->tbuf("fold_G2", 24 * m, &G[1]));
    RET(c->tbuf("fold_eqb", 3 * m, &eqb));
    RET(c->tbuf("fold_zz", (size_t)P.t * 24 * n, &zz));
    RET(c->tbuf("sb_round_partial", sb_round_partial_words(), &partial));
    RET(c->tbuf("round_partial", round_partial_words(), &partial_g));
    RET(c->tbuf("sb_round_out", sb_round_out_words() + 5 * 24, &od));
    // G = sum_j M_j (sum_k zeta_k^{j+1} z_k) + sum_k sum_d alpha_k^{d+1} fhat_{k,d}
    for (int sd = 0; sd < 2; sd++) {
        launch_lincomb_z(c->dcrt, S[sd].z, n, K, d_zp + (size_t)sd * K * P.t, P.t, n, zz, c->stream());
        if (c->ccs_general) {
            u64 *zaos;
            RET(c->tbuf("spmv_zaos_L", (size_t)P.t * n * 24, &zaos));
            launch_spmv_rows(c->dcrt, P.t, c->d_rowptr.data(), c->d_col.data(), c->d_val.data(), zz, (size_t)24 * n, n, zaos, G[sd], m, 0, c->stream());
        } else
            launch_spmv_sum(c->dcrt, P.t, c->d_rowptr.data(), c->d_col.data(), c->d_val.data(), zz, (size_t)24 * n, n, G[sd], m, c->stream());
        if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
        if (launch_sb_add_fhat_comb(S[sd].D, ldn, N, K, d_ap + (size_t)sd * K * 3, G[sd], m, c->stream()) != 0) return LF_ERR_HIP;
    }
    RET(build_eq_dev(c, beta.data(), P.s, eqb));
    c->ev_end(ph);

    ph = c->ev_begin(14);
    c->sv_round_mask = 0;
    c->fold_split_mask = 0;
    u64 *msgs = proof;
    std::vector<Fq3> pt(P.s);
    { HostTimer ht(c); lfs::sumcheck_prologue<GoldV>(tr, P.s, deg); }
    u64 *F[2], *T5[2];
    RET(c->tbuf("sb_F0", (size_t)K2 * 3 * 24 * (m / 2), &F[0]));
    RET(c->tbuf("sb_F1", (size_t)K2 * 3 * 24 * (m / 4 ? m / 4 : 1), &F[1]));
    RET(c->tbuf("fold_T0", 57 * (m / 2), &T5[0]));
    RET(c->tbuf("fold_T1", 57 * (m / 4 ? m / 4 : 1), &T5[1]));
    FoldRoundArgs a;
    a.eqL = S[0].eq_r; a.eqR = S[1].eq_r; a.eqB = eqb; a.G1 = G[0]; a.G2 = G[1]; a.ld = m; a.n = m;
    a.p0 = 0; a.pcnt = m / 2; a.pF0 = 0;
    const u64 *curF = nullptr;
    size_t ldF = 0;
    std::vector<u64> h(sb_round_out_words() + 5 * 24);
    for (u32 round = 1; round <= P.s; round++) {
        if (round > 1) {
            const Fq3Const r = f3c(pt[round - 2]);
            const size_t nn = a.n / 2;
            u64 *dst = T5[round & 1];   // round 2 -> T5[0] (m/2 entries), round 3 -> T5[1], ...
            if (round == 2) {           // sources are the five separate full-size tables
                launch_fix_many(c->dcrt, a.eqL, a.ld, dst, nn, a.n, 1, r, c->stream());
                launch_fix_many(c->dcrt, a.eqR, a.ld, dst + 3 * nn, nn, a.n, 1, r, c->stream());
                launch_fix_many(c->dcrt, a.eqB, a.ld, dst + 6 * nn, nn, a.n, 1, r, c->stream());
                launch_fix_many(c->dcrt, a.G1, a.ld, dst + 9 * nn, nn, a.n, 8, r, c->stream());
                launch_fix_many(c->dcrt, a.G2, a.ld, dst + 33 * nn, nn, a.n, 8, r, c->stream());
                if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
                if (launch_sb_materialize(c->dcrt, S[0].D, S[1].D, ldn, N, m, K, r, F[0], c->stream()) != 0) return LF_ERR_HIP;
                curF = F[0]; ldF = nn;
            } else {
                u64 *fd = F[(round & 1) ? 1 : 0];
                launch_fix_many(c->dcrt, a.eqL, a.ld, dst, nn, a.n, 19, r, c->stream());
                launch_fix_many(c->dcrt, curF, ldF, fd, ldF / 2, ldF, K2 * 3 * 8, r, c->stream());
                if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
                curF = fd; ldF = ldF / 2;
            }
            a.eqL = dst; a.eqR = dst + 3 * nn; a.eqB = dst + 6 * nn; a.G1 = dst + 9 * nn; a.G2 = dst + 33 * nn;
            a.ld = nn; a.n = nn; a.pcnt = nn / 2;
        }
        size_t ev = c->ev_begin(0);
        if (launch_sb_round(c->dcrt, P.b, a, curF, ldF, S[0].D, S[1].D, ldn, N, K, d_mu, partial, od, c->stream()) != 0) return LF_ERR_HIP;
        launch_fold_round_g(c->dcrt, a, partial_g, od + sb_round_out_words(), c->stream());
        if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
        c->ev_end(ev);
        RET(down_small(c, od, h.size(), h.data()));
        u64 *evs = msgs + (size_t)(round - 1) * (deg + 1) * 24;
        HostTimer ht(c);
        sb_compose_message(h.data(), h.data() + sb_round_out_words(), deg, evs);
        pt[round - 1] = lfs::sumcheck_round<GoldV>(tr, evs, deg + 1);
    }
    c->ev_end(ph);

    ph = c->ev_begin(15);
    // theta, eta at r_0 (folding.rs:236-256)
    u64 *theta = proof + (size_t)P.s * (deg + 1) * 24, *eta = theta + (size_t)K2 * 72;
    u64 *eq0, *q, *dpart, *fsm;
    RET(c->tbuf("fold_eq0", 3 * m, &eq0));
    RET(c->tbuf("dec_q", (size_t)P.t * 24 * n, &q));
    RET(c->tbuf("dot_partial", dot_partial_words(K, P.t), &dpart));
    RET(c->tbuf("fold_small", (size_t)K2 * 72 + (size_t)K2 * P.t * 24 + 64, &fsm));
    RET(build_eq_dev(c, pt.data(), P.s, eq0));
    u64 *d_theta = fsm, *d_eta = fsm + (size_t)K2 * 72;
    // theta = f-hat_{k,d}(r_o): the tables of the sumcheck have two entries left, one more fix gives the evaluations (exact arithmetic: the words evaluate_mles gives)
    if (curF && ldF == 2) launch_fix_final(c->dcrt, curF, K2 * 3 * 8, f3c(pt[P.s - 1]), d_theta, c->stream());
    else {
        u64 *sbp;
        RET(c->tbuf("sb_eval_partial", sb_eval_partial_words(K), &sbp));
        for (int sd = 0; sd < 2; sd++)
            if (launch_sb_eval(S[sd].D, ldn, N, eq0, m, K, sbp, d_theta + (size_t)sd * K * 72, c->stream()) != 0) return LF_ERR_HIP;
    }
    for (u32 j = 0; j < P.t; j++) launch_spmv_t_eq(c->dcrt, c->d_colptr[j], c->d_rowidx[j], c->d_valT[j], eq0, m, q + (size_t)j * 24 * n, n, c->stream());
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    for (int sd = 0; sd < 2; sd++) RET(dot_batch_dev(c, S[sd].z, n, K, q, n, P.t, n, dpart, d_eta + (size_t)sd * K * P.t * 24));
    RET(down_small(c, fsm, (size_t)K2 * 72 + (size_t)K2 * P.t * 24, theta));   // theta and eta are contiguous in the proof, as in the buffer
    {
        HostTimer ht(c);
        tr.absorb_ring(theta, (size_t)K2 * 3);
    }
    std::vector<u64> rho_c, rho;
    std::vector<int8_t> rho8;
    {   // get_rhos (folding/utils.rs:116-131)
        HostTimer ht(c);
        tr.absorb_ring(eta, (size_t)K2 * P.t);
        lfs::draw_rho(hv, tr, K2, rho_c, rho, &rho8);
    }
    // f_0 in the coefficient domain -> new witness; Witness::from_f (arith.rs:299-313) behind it on the same stream
    int8_t *d_rho;
    RET(c->tbuf("c_rho", (size_t)K2 * 24 + 64, &d_rho));
    RET(c->h2d_small(d_rho, rho8.data(), rho8.size()));
    int32_t *npl;
    RET(lf_planes_alloc(c, N * 24 * 4, &npl));
    u64 *nf = nullptr, *nw = nullptr;
    const size_t nf_bytes = N * 24 * 8, nw_bytes = (size_t)P.wit_len * 24 * 8;
    RET(lf_planes_alloc(c, nf_bytes, (int32_t **)&nf));
    RET(lf_planes_alloc(c, nw_bytes, (int32_t **)&nw));
    if (launch_sb_fold_witness(S[0].D, S[1].D, ldn, N, K, d_rho, npl, c->stream()) != 0) return LF_ERR_HIP;
    launch_recompose_crt(c->dcrt, npl, N, (u32)N, 1, P.B, 1, 0, nf, N, 0, c->stream());
    launch_recompose_crt(c->dcrt, npl, N, P.wit_len, P.L, P.B, 1, 0, nw, P.wit_len, 0, c->stream());
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    {
        HostTimer ht(c);
        const size_t ll = lf_lcccs_len(&P);
        lfs::fold_instance(hv, P, pt, theta, eta, rho_c.data(), rho.data(), [&](u32 i) { return &S[i / K].lcccs[(size_t)(i % K) * ll * 24]; }, lcccs_out);
    }
    HIPCHK(hipStreamSynchronize(c->stream()));
    *w_out = new lf_witness{c, npl, N, c->device, N * 24 * 4};
    (*w_out)->f_ntt = nf; (*w_out)->f_bytes = nf_bytes; (*w_out)->w_ccs = nw; (*w_out)->w_bytes = nw_bytes;
    c->ev_end(ph);
    return LF_OK;
}
