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

// The stages of FoldStep (lf_ctx.h, lf_fold.cpp) that are the same code as on the b = 2 path -- challenge powers, M z per side, the fix of the special tables,
// the evaluation buffers and the q_j gathers, the finish -- all on this lane's one stream; the f-hat side (digit planes D) and the round kernel are this path's.
int fold_impl_sb(lf_ctx *c, Transcript &tr, SideState *S /* [2] */, u64 *lcccs_out, lf_witness **w_out, u64 *proof) {
    const lf_params &P = c->P;
    if (!sb_base_ok(P.b) || c->sh_world > 1 || !S[0].D || !S[1].D) return LF_ERR_UNSUPPORTED;
    FoldStep f(c, tr, S, proof);
    const size_t m = f.m, N = f.N, ldn = sb_ld(N);
    const u32 K = f.K, K2 = f.K2, deg = f.deg;
    FoldRoundArgs &a = f.a;
    hipStream_t st = c->stream();
    // ---- prepare
    {
        HostTimer ht(c);
        lfs::draw_alpha_zeta<GoldV>(tr, K2, f.alpha, f.zeta);
        lfs::draw_mu_beta<GoldV>(tr, K2, P.s, f.mu, f.beta);
    }
    size_t ph = c->ev_begin(13);
    RET(f.powers_alpha_zeta());
    RET(f.powers_mu());
    RET(f.prepare_buffers());
    u64 *partial, *partial_g, *od;
    RET(c->tbuf("sb_round_partial", sb_round_partial_words(), &partial));
    RET(c->tbuf("round_partial", round_partial_words(), &partial_g));
    RET(c->tbuf("sb_round_out", sb_round_out_words() + 5 * 24, &od));
    // G = sum_j M_j (sum_k zeta_k^{j+1} z_k) + sum_k sum_d alpha_k^{d+1} fhat_{k,d}
    for (int sd = 0; sd < 2; sd++) {
        RET(f.side_mz(sd, st, f.zz, "spmv_zaos_L", 0, f.n));
        if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
        if (launch_sb_add_fhat_comb(S[sd].D, ldn, N, K, f.d_ap + (size_t)sd * K * 3, f.G[sd], m, st) != 0) return LF_ERR_HIP;
    }
    RET(build_eq_dev(c, f.beta.data(), P.s, f.eqb));
    c->ev_end(ph);
    // ---- rounds
    ph = c->ev_begin(14);
    c->sv_round_mask = 0;
    c->fold_split_mask = 0;
    { HostTimer ht(c); lfs::sumcheck_prologue<GoldV>(tr, P.s, deg); }
    u64 *F[2];
    RET(c->tbuf("sb_F0", (size_t)K2 * 3 * 24 * (m / 2), &F[0]));
    RET(c->tbuf("sb_F1", (size_t)K2 * 3 * 24 * (m / 4 ? m / 4 : 1), &F[1]));
    RET(c->tbuf("fold_T0", 57 * (m / 2), &f.T5[0]));
    RET(c->tbuf("fold_T1", 57 * (m / 4 ? m / 4 : 1), &f.T5[1]));
    f.first_tables();
    std::vector<u64> h(sb_round_out_words() + 5 * 24);
    for (u32 round = 1; round <= P.s; round++) {
        if (round > 1) {
            const Fq3Const r = f3c(f.pt[round - 2]);
            const size_t nn = a.n / 2;
            u64 *dst = f.T5[round & 1];   // round 2 -> T5[0] (m/2 entries), round 3 -> T5[1], ...
            f.fix_special(round, r, dst, st);
            if (round == 2) {
                if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
                if (launch_sb_materialize(c->dcrt, S[0].D, S[1].D, ldn, N, m, K, r, F[0], st) != 0) return LF_ERR_HIP;
                f.curF = F[0]; f.ldF = nn;
            } else {
                u64 *fd = F[(round & 1) ? 1 : 0];
                launch_fix_many(c->dcrt, f.curF, f.ldF, fd, f.ldF / 2, f.ldF, K2 * 3 * 8, r, st);
                if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
                f.curF = fd; f.ldF = f.ldF / 2;
            }
            f.set_tables(dst, nn);
            a.pcnt = nn / 2;
        }
        size_t ev = c->ev_begin(0);
        if (launch_sb_round(c->dcrt, P.b, a, f.curF, f.ldF, S[0].D, S[1].D, ldn, N, K, f.d_mu, partial, od, st) != 0) return LF_ERR_HIP;
        launch_fold_round_g(c->dcrt, a, partial_g, od + sb_round_out_words(), st);
        if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
        c->ev_end(ev);
        RET(down_small(c, od, h.size(), h.data()));
        u64 *evs = f.msg(round);
        HostTimer ht(c);
        sb_compose_message(h.data(), h.data() + sb_round_out_words(), deg, evs);
        f.pt[round - 1] = lfs::sumcheck_round<GoldV>(tr, evs, deg + 1);
    }
    c->ev_end(ph);
    // ---- evaluations
    ph = c->ev_begin(15);
    RET(f.eval_buffers());
    // theta = f-hat_{k,d}(r_o): the tables of the sumcheck have two entries left, one more fix gives the evaluations (exact arithmetic: the words evaluate_mles gives)
    if (f.curF && f.ldF == 2) launch_fix_final(c->dcrt, f.curF, K2 * 3 * 8, f3c(f.pt[P.s - 1]), f.d_theta, st);
    else {
        u64 *sbp;
        RET(c->tbuf("sb_eval_partial", sb_eval_partial_words(K), &sbp));
        for (int sd = 0; sd < 2; sd++)
            if (launch_sb_eval(S[sd].D, ldn, N, f.eq0, m, K, sbp, f.d_theta + (size_t)sd * K * 72, st) != 0) return LF_ERR_HIP;
    }
    RET(f.gather_q(st));
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    for (int sd = 0; sd < 2; sd++) RET(dot_batch_dev(c, S[sd].z, f.n, K, f.q, f.n, P.t, f.n, f.dpart, f.d_eta + (size_t)sd * K * P.t * 24));
    RET(down_small(c, f.d_theta, (size_t)K2 * 72 + (size_t)K2 * P.t * 24, f.theta()));   // theta and eta are contiguous in the proof, as in the buffer
    {
        HostTimer ht(c);
        tr.absorb_ring(f.theta(), (size_t)K2 * 3);
    }
    // ---- finish
    RET(f.finish(lcccs_out, w_out, [&](const std::vector<int8_t> &rho8, int8_t *d_rho, int32_t *npl) -> int {
        RET(c->h2d_small(d_rho, rho8.data(), rho8.size()));
        return launch_sb_fold_witness(S[0].D, S[1].D, ldn, N, K, d_rho, npl, st) != 0 ? LF_ERR_HIP : LF_OK;
    }));
    c->ev_end(ph);
    return LF_OK;
}
