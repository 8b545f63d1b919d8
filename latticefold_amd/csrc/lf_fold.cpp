// lf_fold.cpp -- the folding prover (nifs/folding.rs:74-179 with the sumcheck of nifs/folding/utils.rs:273-325) on the GPU kernels, as named stages over one
// state (FoldStep, FoldB2): prepare (challenges; per side combine z, SpMV, f-hat combination; eq tables) -- per round: tail hand-off, fix of the special tables
// (sharded slices, hand-over), choice of the f-hat producer, split decision, kernel dispatch (int8 GEMMs, table rounds, round kernels), collection, completion,
// transcript -- evaluations (theta, eta) -- finish.  The numeric host work is lf_step_host.h's.  Plus the two sumchecks as stand-alone ABI entry points.
#include "lf_ring_host.h"

// Host side of the mailbox protocol of a persistent tail kernel (k_fold_tail / k_lin_tail): per round poll the message, run the transcript
// (unless the device sponge does), write the challenge back.  msgs = slot of the first tail round's message, pt = its challenge.
// after_round (optional): called with the 1-based round number once that round's challenge is known (round0 = number of the first tail round)
static int tail_host_rounds(lf_ctx *c, Transcript &tr, u32 epoch, u32 nr, u32 npts, bool dev_transcript, u64 *msgs, Fq3 *pt,
                            const std::function<void(u32)> *after_round = nullptr, u32 round0 = 0) {
    TailMail *mail = c->tail_mail;
    const auto t_start = std::chrono::steady_clock::now();
    double host_us = 0, wait_us = 0;
    auto t_mark = t_start;
    const bool tl_on = t_tl && t_tl->on;
    for (u32 i = 0; i < nr; i++) {
        u32 spins = 0;
        while (__atomic_load_n(&mail->msg_seq[i], __ATOMIC_ACQUIRE) != epoch) {
            __builtin_ia32_pause();
            if ((++spins & 0xfff) == 0) {
                if (__atomic_load_n(&mail->err, __ATOMIC_RELAXED) == epoch ||
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > 10.0) {
                    __atomic_store_n(&mail->abort_seq, epoch, __ATOMIC_RELEASE);   // the kernel gives up at its next wait
                    (void)hipStreamSynchronize(c->stream());
                    return LF_ERR_HIP;
                }
            }
        }
        if (tl_on) { auto nw = std::chrono::steady_clock::now(); wait_us += std::chrono::duration<double, std::micro>(nw - t_mark).count(); t_mark = nw; }
        u64 *evs = msgs + (size_t)i * npts * 24;
        memcpy(evs, (const void *)mail->msg[i], (size_t)npts * 24 * 8);
        HostTimer ht(c);
        Fq3 r;
        if (dev_transcript) r = fq3_make(mail->chal_out[i][0], mail->chal_out[i][1], mail->chal_out[i][2]);   // drawn by the device sponge
        else r = lfs::sumcheck_round<GoldV>(tr, evs, npts);
        pt[i] = r;
        if (i + 1 < nr && !dev_transcript) {
            mail->chal[i][0] = r.c[0]; mail->chal[i][1] = r.c[1]; mail->chal[i][2] = r.c[2];
            __atomic_store_n(&mail->chal_seq[i], epoch, __ATOMIC_RELEASE);
        }
        if (after_round) (*after_round)(round0 + i);      // (behind the hand-over of the challenge: the device is not kept waiting)
        if (tl_on) { auto nw = std::chrono::steady_clock::now(); host_us += std::chrono::duration<double, std::micro>(nw - t_mark).count(); t_mark = nw; }
    }
    if (dev_transcript) tr.set_state((const u64 *)mail->sponge);   // the host transcript continues where the device sponge stopped
    if (tl_on) fprintf(stderr, "[timeline]    tail: %u rounds, host transcript %.1f us, waiting for the GPU %.1f us\n", nr, host_us, wait_us);
    return LF_OK;
}
// device-transcript mode: hand the sponge to the device (state_out = device [26])
static int tail_sponge_to_device(lf_ctx *c, Transcript &tr, u64 **state_out) {
    RET(c->poseidon_setup());
    *state_out = c->tail_dev_chal + 4 * TAIL_MAX_ROUNDS;   // behind the published challenges (same 4 KB scratch)
    u64 st[26];
    tr.get_state(st);
    HIPCHK(hipMemcpyAsync(*state_out, st, sizeof(st), hipMemcpyHostToDevice, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));   // st is a stack buffer
    return LF_OK;
}
// Tail rounds `round`..s of the linearization sumcheck (k_lin_tail).  cur / cure = the Mz and eq tables of round-1 (n entries, ld n).
int lin_tail_rounds(lf_ctx *c, Transcript &tr, const u64 *cur, const u64 *cure, size_t n, u64 *tout, u64 *partial, u32 round, Fq3 *point,
                           u64 *msgs, u32 deg, const std::function<void(u32)> *after_round) {
    const lf_params &P = c->P;
    RET(c->tail_setup());
    LinTailArgs A;
    A.T = cur; A.E = cure; A.Tout = tout; A.n0 = n; A.rounds = P.s - round + 1; A.deg = deg; A.partial = partial;
    RET(c->tbuf("lin_tail_priv", lin_tail_priv_words(n, P.t), &A.priv));
    A.counters = c->tail_counters; A.dev_chal = c->tail_dev_chal;
    HIPCHK(hipHostGetDevicePointer((void **)&A.mail, c->tail_mail, 0));
    if (++c->tail_epoch >= (1u << 30)) c->tail_epoch = 1;
    A.epoch = c->tail_epoch;
    A.r_first = f3c(point[round - 2]);
    A.dev_transcript = (c->tn.device_transcript && !c->xb.on) ? 1u : 0u;   // the device sponge absorbs internal-basis words
    A.pos_ark = A.pos_mds = nullptr; A.sponge_state = nullptr;
    if (A.dev_transcript) {
        RET(tail_sponge_to_device(c, tr, &A.sponge_state));
        A.pos_ark = c->d_poseidon; A.pos_mds = c->d_poseidon + 720;
    }
    if (launch_lin_tail(c->dcrt, c->desc, A, c->stream()) == 0) return LF_ERR_UNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    return tail_host_rounds(c, tr, A.epoch, A.rounds, deg + 1, A.dev_transcript != 0, msgs + (size_t)(round - 1) * (deg + 1) * 24, &point[round - 1], after_round, round);
}
// Tail rounds `round`..s of the folding sumcheck in one persistent kernel (lf_kernels.hip: k_fold_tail).  On entry `a` / `curF`
// describe the tables of round-1 (a.n entries each, leading dimension a.n) and pt[round-2] is the challenge that fixes them.
// The host side of the mailbox protocol: poll the message of a round, run the transcript, write the challenge back.
static int fold_tail_rounds(lf_ctx *c, Transcript &tr, const FoldRoundArgs &a, u64 *curF, u64 *const Fbuf[2], u64 *T_other, const Fq3Const *d_mu,
                            u64 *partial, u32 round, std::vector<Fq3> &pt, u64 *msgs, u32 deg) {
    const lf_params &P = c->P;
    RET(c->tail_setup());
    const u32 nr = P.s - round + 1;
    FoldTailArgs A;
    A.T[0] = (u64 *)a.eqL; A.T[1] = T_other;
    A.F[0] = curF; A.F[1] = curF == Fbuf[0] ? Fbuf[1] : Fbuf[0];
    A.n0 = a.n; A.rounds = nr; A.K = P.K; A.mu_pow = d_mu; A.partial = partial;
    A.counters = c->tail_counters; A.dev_chal = c->tail_dev_chal;
    RET(c->tbuf("tail_eqpriv", fold_tail_eqpriv_words(a.n, P.K), &A.eqpriv));
    HIPCHK(hipHostGetDevicePointer((void **)&A.mail, c->tail_mail, 0));
    if (++c->tail_epoch >= (1u << 30)) c->tail_epoch = 1;
    A.epoch = c->tail_epoch;
    A.r_first = f3c(pt[round - 2]);
    A.dev_transcript = (c->tn.device_transcript && !c->xb.on) ? 1u : 0u;   // the device sponge absorbs internal-basis words
    A.pos_ark = A.pos_mds = nullptr; A.sponge_state = nullptr;
    if (A.dev_transcript) {   // LF_DEVICE_TRANSCRIPT=1: hand the sponge to the device for the tail rounds
        RET(tail_sponge_to_device(c, tr, &A.sponge_state));
        A.pos_ark = c->d_poseidon; A.pos_mds = c->d_poseidon + 720;
    }
    if (launch_fold_tail(c->dcrt, A, c->num_cus, c->stream()) == 0) return LF_ERR_UNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    return tail_host_rounds(c, tr, A.epoch, nr, deg + 1, A.dev_transcript != 0, msgs + (size_t)(round - 1) * (deg + 1) * 24, &pt[round - 1]);
}

// ---- LFFoldingProver::prove (nifs/folding.rs:42-130) as stages over one state ----------------------------------------------------------------------
// FoldStep (lf_ctx.h) is what the b = 2 driver below and the small-base driver (lf_fold_sb.cpp) share; its members are the stages that are the same code on both
// paths.  They queue on the stream they are given: which streams a path uses is that path's schedule.
FoldStep::FoldStep(lf_ctx *c_, Transcript &tr_, SideState *S_, u64 *proof_)
    : c(c_), tr(tr_), S(S_), proof(proof_), P(c_->P), m(c_->m), n(c_->n), N(c_->N), K(c_->P.K), K2(2 * c_->P.K), deg(2 * c_->P.b), hv{c_->ring}, pt(c_->P.s) {}
// powers x^{j+1} of the challenges, as the kernels take them
int FoldStep::powers_alpha_zeta() {
    std::vector<Fq3Const> a_pow((size_t)K2 * 3), z_pow((size_t)K2 * P.t);
    for (u32 i = 0; i < K2; i++) {
        lfs::powers(hv, alpha[i], 3, [&](u32 d, const Fq3 &pw) { a_pow[(size_t)i * 3 + d] = f3c(pw); });
        lfs::powers(hv, zeta[i], P.t, [&](u32 j, const Fq3 &pw) { z_pow[(size_t)i * P.t + j] = f3c(pw); });
    }
    RET(upload_consts(c, "c_ap", a_pow, &d_ap));
    return upload_consts(c, "c_zp", z_pow, &d_zp);
}
int FoldStep::powers_mu() {
    std::vector<Fq3Const> mu_pow((size_t)K2 * 3);
    for (u32 i = 0; i < K2; i++) lfs::powers(hv, mu[i], 3, [&](u32 d, const Fq3 &pw) { mu_pow[(size_t)i * 3 + d] = f3c(pw); });
    return upload_consts(c, "c_mu", mu_pow, &d_mu);
}
int FoldStep::prepare_buffers() {
    RET(c->tbuf("fold_G1", 24 * m, &G[0]));
    RET(c->tbuf("fold_G2", 24 * m, &G[1]));
    RET(c->tbuf("fold_eqb", 3 * m, &eqb));
    return c->tbuf("fold_zz", (size_t)P.t * 24 * n, &zz);
}
// rows [g_r0, g_r0 + g_rcnt) of G_sd = sum_j M_j (sum_k zeta_k^{j+1} z_k) on `st`, through the columns [zc_lo, zc_hi) of zb; the caller adds the f-hat combination
int FoldStep::side_mz(int sd, hipStream_t st, u64 *zb, const char *zaos_name, size_t zc_lo, size_t zc_hi, size_t g_r0, size_t g_rcnt) {
    launch_lincomb_z(c->dcrt, S[sd].z + zc_lo, n, K, d_zp + (size_t)sd * K * P.t, P.t, zc_hi - zc_lo, zb + zc_lo, st);
    if (c->ccs_general) {
        u64 *zaos;
        RET(c->tbuf(zaos_name, (size_t)P.t * n * 24, &zaos));
        launch_spmv_rows(c->dcrt, P.t, c->d_rowptr.data(), c->d_col.data(), c->d_val.data(), zb, (size_t)24 * n, n, zaos, G[sd], m, 0, st, g_r0, g_rcnt);
    } else
        launch_spmv_sum(c->dcrt, P.t, c->d_rowptr.data(), c->d_col.data(), c->d_val.data(), zb, (size_t)24 * n, n, G[sd], m, st, g_r0, g_rcnt);
    return LF_OK;
}
void FoldStep::first_tables() {   // round 1: the five separate full-size tables
    a.eqL = S[0].eq_r; a.eqR = S[1].eq_r; a.eqB = eqb; a.G1 = G[0]; a.G2 = G[1]; a.ld = m; a.n = m;
    a.p0 = 0; a.pcnt = m / 2; a.pF0 = 0;
}
void FoldStep::set_tables(u64 *dst, size_t nn) {   // the 57-plane buffer: eqL[3] eqR[3] eqB[3] G1[24] G2[24]
    a.eqL = dst; a.eqR = dst + 3 * nn; a.eqB = dst + 6 * nn; a.G1 = dst + 9 * nn; a.G2 = dst + 33 * nn;
    a.ld = nn; a.n = nn;
}
// the special tables of round-1, fixed at `r` into dst (whole tables).  eqB always on the caller's stream; the other four on sg, which may be the second stream
// of a GEMM round (the norm part needs eqB only, the G part the other four tables)
void FoldStep::fix_special(u32 round, Fq3Const r, u64 *dst, hipStream_t sg) {
    const size_t nn = a.n / 2;
    if (round == 2) {   // sources are the five separate full-size tables
        launch_fix_many(c->dcrt, a.eqL, a.ld, dst, nn, a.n, 1, r, sg);
        launch_fix_many(c->dcrt, a.eqR, a.ld, dst + 3 * nn, nn, a.n, 1, r, sg);
        launch_fix_many(c->dcrt, a.eqB, a.ld, dst + 6 * nn, nn, a.n, 1, r, c->stream());
        launch_fix_many(c->dcrt, a.G1, a.ld, dst + 9 * nn, nn, a.n, 8, r, sg);
        launch_fix_many(c->dcrt, a.G2, a.ld, dst + 33 * nn, nn, a.n, 8, r, sg);
    } else if (sg != c->stream()) {   // the 57-plane buffer in three pieces: eqL eqR | eqB | G1 G2
        launch_fix_many(c->dcrt, a.eqL, a.ld, dst, nn, a.n, 2, r, sg);
        launch_fix_many(c->dcrt, a.eqB, a.ld, dst + 6 * nn, nn, a.n, 1, r, c->stream());
        launch_fix_many(c->dcrt, a.G1, a.ld, dst + 9 * nn, nn, a.n, 16, r, sg);
    } else {            // source is the previous 57-plane buffer (same layout): one launch over its 19 F_{p^3} rows
        launch_fix_many(c->dcrt, a.eqL, a.ld, dst, nn, a.n, 19, r, c->stream());
    }
}
// theta, eta at r_0 (folding.rs:236-256): their buffers and eq(r_o)
// (q_words = false: the caller gathers q_j straight into the packed digits -- q_pack_dev -- and the words get no buffer)
int FoldStep::eval_buffers(bool q_words) {
    u64 *fsm;
    RET(c->tbuf("fold_eq0", 3 * m, &eq0));
    if (q_words) RET(c->tbuf("dec_q", (size_t)P.t * 24 * n, &q));
    RET(c->tbuf("dot_partial", dot_partial_words(K, P.t), &dpart));
    RET(c->tbuf("fold_small", (size_t)K2 * 72 + (size_t)K2 * P.t * 24 + 64, &fsm));
    d_theta = fsm; d_eta = fsm + (size_t)K2 * 72;   // contiguous, as theta and eta are in the proof
    return build_eq_dev(c, pt.data(), P.s, eq0);
}
// q_j = M_j^T eq(r_o), every second one on s1f (the gathers are latency-bound: 3 x 63 us in a row at C4)
int FoldStep::gather_q(hipStream_t s1f) {
    size_t c0, cnt;
    shard_slice(c, n, &c0, &cnt);   // (sharded: the eta inner products read this rank's column slice of q_j only)
    if (P.t > 1) RET(c->fork(c->stream(), s1f));           // eq(r_o) is built
    for (u32 j = 0; j < P.t; j++)
        launch_spmv_t_eq(c->dcrt, c->d_colptr[j], c->d_rowidx[j], c->d_valT[j], eq0, m, q + (size_t)j * 24 * n, n, (j & 1) ? s1f : c->stream(), c0, cnt);
    if (P.t > 1) RET(c->join(s1f, c->stream()));
    return LF_OK;
}
// Finish: eta into the transcript, rho (get_rhos, folding/utils.rs:116-131), the folded witness f_0 in the coefficient domain -- fold_witness(rho8, d_rho, npl)
// uploads rho and launches the path's kernel -- Witness::from_f (arith.rs:299-313) behind it on the same stream, and the folded instance
// (folding/utils.rs:460-521) on the host while the GPU folds the witness.
int FoldStep::finish(u64 *lcccs_out, lf_witness **w_out, const std::function<int(const std::vector<int8_t> &, int8_t *, int32_t *)> &fold_witness) {
    std::vector<u64> rho_c, rho;
    std::vector<int8_t> rho8;
    {
        HostTimer ht(c);
        tr.absorb_ring(eta(), (size_t)K2 * P.t);
        lfs::draw_rho(hv, tr, K2, rho_c, rho, &rho8);
    }
    int8_t *d_rho;
    RET(c->tbuf("c_rho", (size_t)K2 * 24 + 64, &d_rho));
    int32_t *npl;
    RET(lf_planes_alloc(c, N * 24 * 4, &npl));
    RET(fold_witness(rho8, d_rho, npl));
    // f = CRT(f_coeff) and w_ccs = CRT(recompose(f_coeff, B, L)) of the folded witness, behind compute_f_0
    u64 *nf = nullptr, *nw = nullptr;
    const size_t nf_bytes = N * 24 * 8, nw_bytes = (size_t)P.wit_len * 24 * 8;
    RET(lf_planes_alloc(c, nf_bytes, (int32_t **)&nf));
    RET(lf_planes_alloc(c, nw_bytes, (int32_t **)&nw));
    launch_recompose_crt(c->dcrt, npl, N, (u32)N, 1, P.B, 1, 0, nf, N, 0, c->stream());
    launch_recompose_crt(c->dcrt, npl, N, P.wit_len, P.L, P.B, 1, 0, nw, P.wit_len, 0, c->stream());
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    LF_TRACE(c, "fold_witness");
    TL_MARK("  eta absorbed, rho drawn, fold_witness enqueued");
    {
        HostTimer ht(c);
        const size_t ll = lf_lcccs_len(&P);
        lfs::fold_instance(hv, P, pt, theta(), eta(), rho_c.data(), rho.data(), [&](u32 i) { return &S[i / K].lcccs[(size_t)(i % K) * ll * 24]; }, lcccs_out);
    }
    TL_MARK("  folded instance on the host");
    HIPCHK(hipStreamSynchronize(c->stream()));
    *w_out = new lf_witness{c, npl, N, c->device, N * 24 * 4};
    (*w_out)->f_ntt = nf; (*w_out)->f_bytes = nf_bytes; (*w_out)->w_ccs = nw; (*w_out)->w_bytes = nw_bytes;
    TL_MARK(" rho + fold_witness");
    return LF_OK;
}
// Round 2 (round 1 only on request: its integer kernel is faster than the gathers) as table look-ups: the coefficient quadruples of h^3 - h for the 9 / 81
// digit codes of a pair, [code][4][3] words.  The entries of a pair are digits in round 1, d_a + (d_b - d_a) r1 in round 2.
static void fold_tab_poly(const GoldV &hv, u32 round, const Fq3 &r1v, std::vector<u64> &poly) {
    const int nd = round == 1 ? 2 : 4, ncode = round == 1 ? 9 : 81;
    poly.assign((size_t)ncode * 12, 0);
    const Fq3 one = fq3_one();
    auto small = [&](int v) { return v == 0 ? fq3_zero() : (v > 0 ? (v == 1 ? one : fq3_add(one, one)) : (v == -1 ? fq3_neg(one) : fq3_neg(fq3_add(one, one)))); };
    for (int code = 0; code < ncode; code++) {
        int dg[4] = {0, 0, 0, 0}, cc = code;
        for (int b = 0; b < nd; b++, cc /= 3) dg[b] = cc % 3 - 1;
        Fq3 f0, f1;
        if (round == 1) { f0 = small(dg[0]); f1 = small(dg[1]); }
        else {
            f0 = fq3_add(small(dg[0]), hv.ext_mul(small(dg[1] - dg[0]), r1v));
            f1 = fq3_add(small(dg[2]), hv.ext_mul(small(dg[3] - dg[2]), r1v));
        }
        Fq3 df = fq3_sub(f1, f0), f0s = hv.ext_mul(f0, f0), dfs = hv.ext_mul(df, df);
        Fq3 t1 = hv.ext_mul(f0s, df), t2 = hv.ext_mul(f0, dfs);
        Fq3 q[4] = {fq3_sub(hv.ext_mul(f0s, f0), f0), fq3_sub(fq3_add(fq3_add(t1, t1), t1), df), fq3_add(fq3_add(t2, t2), t2), hv.ext_mul(dfs, df)};
        for (int e = 0; e < 4; e++)
            for (int w = 0; w < 3; w++) poly[(size_t)code * 12 + 3 * e + w] = q[e].c[w];
    }
}
// The b = 2 driver (stages: file header)
struct FoldB2 : FoldStep {
    using FoldStep::FoldStep;
    const size_t Gw = (size_t)c->sh_world, gr = (size_t)c->sh_rank;
    // switches of this step (prepare, rounds_begin)
    bool sv_split = false, fr_split = false, fused = false, use_lut = false, use_r4tab = false, use_r5 = false, use_sv = false, sv_two_streams = false;
    // what the round loop mutates
    bool sharded = false;
    int flip = 0, fmode = 0;       // fmode: producer of this round's pairs: 0 tables, 1 fused fix, 3 / 4 digit look-up table (rounds 3 / 4), 7 round 5 from the planes
    const u64 *prevF = nullptr;    // (mode 1) the tables the fused fix reads, leading dimension prevld
    size_t prevld = 0, ldEr = 0;
    u64 *svE[3] = {nullptr, nullptr, nullptr}, *svE_rest = nullptr;   // E_1 .. E_3, and E_l for l >= 4 in one buffer
    u32 svE_level = 1;             // E_1 .. E_level exist
    lfs::SplitCoef<GoldV> sp{};    // c_i = prod_{k<i} eq(beta_k, r_k), beta_i and their inverses of a split round
    bool split_now = false;
    const u64 *Er = nullptr;       // (split round) E_round, leading dimension ldEr
    u64 *F[2] = {nullptr, nullptr}, *partial = nullptr, *od = nullptr, *od_host = nullptr, *od_shard = nullptr, *d_lut = nullptr;
    u32 *sv_bits[2] = {nullptr, nullptr};
    hipStream_t sv_g_stream = nullptr;

    u64 *svE_ptr(u32 l) const {
        if (l <= 3) return svE[l - 1];
        size_t off = 0;
        for (u32 q = 4; q < l; q++) off += 3 * (m >> q);
        return svE_rest + off;
    }
    void svE_ensure(u32 l) {   // E_{q+1} = pair sums of E_q
        for (; svE_level < l; svE_level++)
            launch_eq_pairsum(svE_ptr(svE_level), m >> svE_level, m >> (svE_level + 1), svE_ptr(svE_level + 1), m >> (svE_level + 1), c->stream());
    }
    int prepare(), rounds_begin(), tail_handoff(u32 round, bool *done), fix_tables(u32 round, u64 *dst, bool *gathered), choose_producer(u32 round);
    void decide_split(u32 round);
    int gemm_round(u32 round), dispatch(u32 round), collect(u32 round), rounds(), evaluations();
};

int FoldB2::prepare() {
    { HostTimer ht(c); lfs::draw_alpha_zeta<GoldV>(tr, K2, alpha, zeta); }
    // The G tables need alpha and zeta only: their chains are enqueued HERE, and the host squeezes mu and beta (~100 permutations) while the GPU combines
    // the z_k -- the challenge order of the transcript (alpha, zeta, mu, beta: folding/utils.rs:52-95) is untouched.
    size_t ph = c->ev_begin(13);
    RET(powers_alpha_zeta());
    RET(prepare_buffers());
    RET(c->tbuf("round_partial", round_partial_words(), &partial));
    od = od_host = c->round_out();
    if (!od) return LF_ERR_HIP;
    if (c->sh_world > 1) {   // the round kernels of a sharded step leave their partial message in device memory (exchanged there)
        RET(c->tbuf("fold_round_out", 5 * 24 + 8, &od_shard));
        od = od_shard;
    }
    // sharded from round 1 on (the condition of the round loop): the special tables live as entry slices until the hand-over to the replicated tail --
    // a rank evaluates and fixes only the entries [rank m/G, (rank+1) m/G) of them until they are gathered: only those rows of G, through the columns they read
    const bool shard_tabs = shard_keep(c, 1, m);
    const size_t g_r0 = shard_tabs ? (size_t)c->sh_rank * (m / (size_t)c->sh_world) : 0, g_rcnt = shard_tabs ? m / (size_t)c->sh_world : (size_t)-1;
    size_t zc_lo = 0, zc_hi = n;
    if (shard_tabs) RET(shard_col_range(c, g_r0, g_rcnt, &zc_lo, &zc_hi));
    {
        // G = sum_j M_j (sum_k zeta_k^{j+1} z_k)  +  sum_k sum_d alpha_k^{d+1} fhat_{k,d}: the two sides are independent chains -- the right one runs on
        // the (idle) stream of the helper lane next to the left one: the SpMV gathers of one side overlap the multiply-bound combination of the other
        hipStream_t s0 = c->stream(), s1 = (t_lane == 0) ? c->st_lane[1] : s0;
        u64 *zz1 = zz;
        if (s1 != s0) RET(c->tbuf("fold_zz1", (size_t)P.t * 24 * n, &zz1));
        RET(c->fork(s0, s1));           // the challenge powers were uploaded on s0
        // one-entry-per-row matrices, t <= 4, whole tables: both sums in ONE pass that writes each row of G once (k_g_rows) and does not look up the trailing
        // empty rows of the matrices; otherwise G = M zb (k_spmv_rows / k_spmv_sum), then read back and completed by k_add_fhat_comb
        const bool one_pass = !c->tn.no_live_rows && !c->ccs_general && P.t <= 4 && !shard_tabs && c->sh_world == 1 && N <= m;
        for (int sd = 0; sd < 2; sd++) {
            hipStream_t st = sd ? s1 : s0;
            if (one_pass) {
                u64 *zb = sd ? zz1 : zz;
                launch_lincomb_z(c->dcrt, S[sd].z, n, K, d_zp + (size_t)sd * K * P.t, P.t, n, zb, st);
                launch_g_rows(c->dcrt, P.t, c->d_rowptr.data(), c->d_col.data(), c->d_val.data(), zb, (size_t)24 * n, n, c->live_rows, S[sd].planes, N, K,
                              d_ap + (size_t)sd * K * 3, G[sd], m, st);
                continue;
            }
            RET(side_mz(sd, st, sd ? zz1 : zz, sd ? "spmv_zaos_R" : "spmv_zaos_L", zc_lo, zc_hi, g_r0, g_rcnt));
            launch_add_fhat_comb(c->dcrt, S[sd].planes, N, K, d_ap + (size_t)sd * K * 3, G[sd], m, st, g_r0, g_rcnt);
        }
        RET(c->join(s1, s0));
    }
    { HostTimer ht(c); lfs::draw_mu_beta<GoldV>(tr, K2, P.s, mu, beta); }
    TL_MARK(" fold challenges");
    RET(powers_mu());
    RET(build_eq_dev(c, beta.data(), P.s, eqb));
    // split form of the GEMM rounds (lf_sv_rounds.h): eqB fixed at r_1..r_{i-1} is c_i eq(beta_i, b) E_i[p] at entry 2p + b, E_i = eq((beta_{i+1}..beta_s), .) -- one
    // value per pair, so the GEMM of round i runs against 24 digit columns instead of 48.  E_1 here, E_2 / E_3 as pair sums when their round comes.
    sv_split = !c->tn.fold_sv_no_split && P.s >= 4 && m >= 256;
    if (sv_split) {
        RET(c->tbuf("fold_svE1", 3 * (m / 2), &svE[0]));
        RET(c->tbuf("fold_svE2", 3 * (m / 4), &svE[1]));
        RET(c->tbuf("fold_svE3", 3 * (m / 8), &svE[2]));
        RET(build_eq_dev(c, beta.data() + 1, P.s - 1, svE[0]));
    }
    // the same form in the large table rounds after the GEMMs (k_fold_round SPLIT: three lazy products per table instead of four, the host completes the message)
    fr_split = sv_split && c->sh_world == 1 && c->dcrt.nu2p40 && !c->tn.fold_rounds_no_split;
    if (fr_split) RET(c->tbuf("fold_svE_rest", 3 * (m / 8) + 64, &svE_rest));
    LF_TRACE(c, "fold prepare");
    c->ev_end(ph);
    if (t_tl && t_tl->on) { (void)hipStreamSynchronize(c->stream()); TL_MARK(" fold prepare (synced)"); }
    return LF_OK;
}
// the switches of the round loop and its working tables
int FoldB2::rounds_begin() {
    sharded = Gw > 1;
    // Rounds >= 4 with many pairs: fix_variables of the f-hat tables is fused into the (ALU-bound) round kernel,
    // so the separate memory-bound pass over them vanishes (rounds 4-6 at 2^20 rows: 6.25 -> 5.6 ms).
    fused = !c->tn.fold_unfused && (Gw == 1 || !c->tn.shard_plain_rounds);   // (sharded: the kernels offset their table pointers by the rank's first pair)
    // Rounds 3 and 4 of large unsharded instances never materialise the m/4-entry tables: their entries are one of 81 values
    // (four ternary digits) and come from a look-up table in LDS (k_fold_round modes 3 and 4); P.s >= 4 and m/4 >= lut_min entries
    // (default 2^14, measured: C2 6.65 -> 6.52 ms, 2^18 rows 10.7 -> 9.6 ms against 2^17).
    use_lut = fused && P.s >= 4 && m / 4 >= c->tn.lut_min && m / 4 >= 4 && !c->tn.fold_no_lut;
    // rounds 4 and 5 from product-free tables over the digit codes (k_fold_round modes 6 and 7); with round 5 on the planes too, round 4 stores no tables
    use_r4tab = use_lut && c->dcrt.nu2p40 && !c->tn.fold_no_r4tab;
    // (not when the persistent tail may take over at round 5: it starts from the materialised round-4 tables)
    use_r5 = use_r4tab && !c->tn.fold_no_r5tab && Gw == 1 && P.s >= 5 && (N & 3) == 0 && (c->tn.no_tail || m / 8 > c->tn.tail_n) && m / 32 >= c->tn.r5_min;
    // f-hat is materialised after two rounds (m/4 entries, F[0]; round r > 3 writes its m/2^(r-1) entries to F[r odd ? 0 : 1]) -- or later: the
    // look-up-table rounds store their first tables in round 4 (m/8, F[1]), with round 5 on the planes too in round 5 (m/16, F[0]).  Sized
    // for what this step will write: 6.8 GiB -> 1.4 GiB at 2^20 rows.
    const size_t half = m / 2, f0_ent = use_lut ? m / 16 : m / 4, f1_ent = use_r5 ? m / 32 : m / 8;
    RET(c->tbuf("fold_F0", (size_t)K2 * 3 * 24 * (f0_ent ? f0_ent : 1), &F[0]));
    RET(c->tbuf("fold_F1", (size_t)K2 * 3 * 24 * (f1_ent ? f1_ent : 1), &F[1]));
    RET(c->tbuf("fold_T0", 57 * (half ? half : 1), &T5[0]));
    RET(c->tbuf("fold_T1", 57 * (half / 2 ? half / 2 : 1), &T5[1]));
    first_tables();
    c->sv_round_mask = 0;
    c->fold_split_mask = 0;
    sv_two_streams = t_lane == 0 && Gw == 1;
    sv_g_stream = c->stream();
    use_sv = !c->tn.force_exchange && !c->tn.fold_no_sv && (Gw == 1 || !c->tn.shard_plain_rounds) && N <= m && (N & 3) == 0 && !c->tn.fold_tab_r1;
    return LF_OK;
}
// Persistent tail: once the materialised tables are small, ONE kernel runs all remaining rounds and exchanges messages / challenges with this thread through
// a host-mapped mailbox (k_fold_tail) -- no launches and no stream sync per round.  (A sharded step: once its tables are replicated, every rank runs its own tail.)
int FoldB2::tail_handoff(u32 round, bool *done) {
    if (sharded || c->tn.no_tail || round < 5 || !curF || ldF != a.n || a.n > c->tn.tail_n || a.n < 4 || P.s - round + 1 > TAIL_MAX_ROUNDS) return LF_OK;
    int trc = fold_tail_rounds(c, tr, a, (u64 *)curF, F, T5[flip], d_mu, partial, round, pt, proof, deg);
    if (trc == LF_OK) {
        curF = (u64 *)curF == F[0] ? F[1] : F[0];   // the tail leaves the fully fixed tables (2 entries per row) in the other buffer
        ldF = 2;
        *done = true;
    }
    return trc == LF_ERR_UNSUPPORTED ? LF_OK : trc;   // LF_ERR_UNSUPPORTED: not launchable here -> ordinary rounds
}
// Sharded rounds: rank g evaluates the pairs of its index slice (high bits: pairs (2j,2j+1) stay local, the f-hat tables exist only for that
// slice), the (D+1)-element partial messages are all-gathered and added mod p, every rank runs the same transcript.  Once fewer than 64 pairs per rank remain
// the slices are gathered and the rounds from there on are replicated: *gathered says that this hand-over took the f-hat tables along (rounds > 3).
int FoldB2::fix_tables(u32 round, u64 *dst, bool *gathered) {
    const Fq3Const r = f3c(pt[round - 2]);
    const size_t nn = a.n / 2;
    const bool handover = sharded && !shard_keep(c, 1, nn);   // this round's fix is the last one on slices
    // GEMM rounds: the fixes of the four tables of the G part (and the G kernel) run on the helper lane's idle stream next to the GEMM chain
    hipStream_t sg = c->stream();
    if (use_sv && sv_two_streams && !sharded && (int)round <= c->tn.sv_rounds && round <= 3 && nn / 2 >= c->tn.sv_min && sv_shape_ok(1 << (round - 1), nn / 2, K))
        sg = c->st_lane[1];
    sv_g_stream = sg;
    if (!sharded) { fix_special(round, r, dst, sg); return LF_OK; }
    // this rank's entries [rank nn/G, (rank+1) nn/G) of the new tables come from its own entries of the old ones
    const size_t j0 = gr * (nn / Gw), jc = nn / Gw;
    if (round == 2) {
        launch_fix_many(c->dcrt, a.eqL + 2 * j0, a.ld, dst + j0, nn, 2 * jc, 1, r, sg);
        launch_fix_many(c->dcrt, a.eqR + 2 * j0, a.ld, dst + 3 * nn + j0, nn, 2 * jc, 1, r, sg);
        launch_fix_many(c->dcrt, a.eqB + 2 * j0, a.ld, dst + 6 * nn + j0, nn, 2 * jc, 1, r, sg);
        launch_fix_many(c->dcrt, a.G1 + 2 * j0, a.ld, dst + 9 * nn + j0, nn, 2 * jc, 8, r, sg);
        launch_fix_many(c->dcrt, a.G2 + 2 * j0, a.ld, dst + 33 * nn + j0, nn, 2 * jc, 8, r, sg);
    } else {
        launch_fix_many(c->dcrt, a.eqL + 2 * j0, a.ld, dst + j0, nn, 2 * jc, 19, r, sg);
    }
    if (!handover) return LF_OK;
    sharded = false;
    if (round <= 3) return gather_slices(c, dst, 57, nn);   // the f-hat tables are still virtual: the special tables alone
    // the 57 special planes and the fixed f-hat slices in ONE all-gather (RCCL over xGMI), interleaved into full tables
    u64 *fd = F[(round & 1) ? 0 : 1];
    const size_t lcl = ldF / 2;  // local entries after this fix
    launch_fix_many(c->dcrt, curF, ldF, fd, lcl, ldF, K2 * 3 * 8, r, c->stream());
    // fd is source (local layout [planes][lcl]) and destination (full tables, the parity an ordinary fix output has: the ping-pong of the following rounds stays valid)
    const GatherPart gp[2] = {{dst + gr * lcl, nn, dst, 57}, {fd, lcl, fd, (size_t)K2 * 3 * 24}};
    RET(gather_parts(c, gp, 2, lcl));
    curF = fd; ldF = nn;
    *gathered = true;
    return LF_OK;
}
// where this round's f-hat pairs come from (fmode), and the tables it leaves behind (curF, ldF)
int FoldB2::choose_producer(u32 round) {
    const size_t nn = a.n / 2;
    if (round == 3) {
        const size_t q = sharded ? nn / Gw : nn, j0 = sharded ? gr * q : 0;   // this rank's slice of the m/4 entries
        if (use_lut) {
            Fq3 lut[162];
            lfs::fold_lut81(hv, pt[0], pt[1], lut);
            RET(c->tbuf("fold_lut", 2 * 81 * 3 + 8, &d_lut));
            RET(c->h2d_small(d_lut, lut, sizeof(lut)));   // (an Fq3 is its three words)
            fmode = 3;
            curF = nullptr; ldF = q;
        } else {
            Fq3 Wf[4];
            lfs::eq_weights(hv, pt.data(), 2, Wf);   // W_b = eq((r1, r2), b)
            const Fq3Const W[4] = {f3c(Wf[0]), f3c(Wf[1]), f3c(Wf[2]), f3c(Wf[3])};
            launch_fold_materialize2(c->dcrt, S[0].planes, S[1].planes, N, j0, q, K, W, F[0], c->stream());
            curF = F[0]; ldF = q;
        }
    } else if (round > 3) {
        u64 *fd = F[(round & 1) ? 0 : 1];  // round 4 -> F[1], round 5 -> F[0], ...
        if (use_lut && round == 4) fmode = 4;
        else if (use_r5 && round == 5) fmode = 7;
        else if (fused && ldF >= c->tn.fuse_min && ldF >= 4) { prevF = curF; prevld = ldF; fmode = 1; }   // (fuse_min entries, measured: 65536 -> 16384 = -0.3 ms at 2^20 rows)
        else launch_fix_many(c->dcrt, curF, ldF, fd, ldF / 2, ldF, K2 * 3 * 8, f3c(pt[round - 2]), c->stream());
        curF = fd; ldF = ldF / 2;
    }
    return LF_OK;
}
// split form of this round's kernel?  (modes 6, 7; c_i and beta_i must be invertible for the host's completion.  Mode 1, the fused-fix rounds after them,
// measured slower in this form: 0.55 against 0.51 ms per launch at C4 -- its four reduced products per table dominate)
void FoldB2::decide_split(u32 round) {
    Er = nullptr; ldEr = 0; split_now = false;
    if (!(fr_split && round >= 2 && !sharded && (fmode == 7 || (fmode == 4 && use_r4tab)) && a.pcnt >= c->tn.fold_split_min)) return;
    sp = lfs::split_coef(hv, lfs::eq_prefix(hv, beta.data(), pt.data(), round), beta[round - 1]);
    if (!sp.ok) return;
    svE_ensure(round);
    Er = svE_ptr(round); ldEr = m >> round;
    split_now = true;
    c->fold_split_mask |= 1u << (round - 1);
}
// rounds 1..3 as exact int8 GEMMs on the matrix cores (lf_sv_rounds.h): G part on the VALU, norm part from the witness planes
int FoldB2::gemm_round(u32 round) {
    const int svV = 1 << (round - 1);
    std::vector<Fq3> W((size_t)svV), Cf;   // W_b = eq((r_1..r_{i-1}), b); C_pi(X) -> [pairs][4][3] internal-basis words
    lfs::eq_weights(hv, pt.data(), round - 1, W.data());
    lfs::sv_coef(hv, svV, W.data(), sv_num_pairs(svV), [&](int i) { return sv_pair(svV, i); }, Cf);
    u64 *d_coef, *gtmp, *svtp;
    unsigned char *sveb;
    int32_t *svpart, *svtot;
    RET(c->tbuf("sv_coef", Cf.size() * 3 + 8, &d_coef));
    RET(c->tbuf("sv_gtmp", 128, &gtmp));
    RET(c->tbuf("sv_tp", sv_tp_words(K), &svtp));
    RET(c->tbuf("sv_eb", sv_eb_bytes(a.pcnt), &sveb));
    RET(c->tbuf("sv_part", sv_part_words(svV, a.pcnt, K), &svpart));
    RET(c->tbuf("sv_tot", sv_tot_words(svV, K), &svtot));
    RET(c->h2d_small(d_coef, Cf.data(), Cf.size() * sizeof(Fq3)));   // (an Fq3 is its three words)
    if (!sv_bits[0])   // bit-plane form of the two witnesses, once per step (the fold step builds it ahead on the other lane)
        for (int sd = 0; sd < 2; sd++) {
            if (S[sd].sv_bits) { sv_bits[sd] = S[sd].sv_bits; continue; }
            RET(c->tbuf(sd ? "sv_bits_R" : "sv_bits_L", sv_bits_words(N, K), &sv_bits[sd]));
            if (launch_sv_bits(S[sd].planes, N, N, K, sv_bits[sd], c->stream()) < 0) return LF_ERR_HIP;
        }
    hipStream_t sg = round == 1 ? (sv_two_streams && !sharded ? c->st_lane[1] : c->stream()) : sv_g_stream;
    // the tables of round 1 come from fold prepare, whose left chain ran on this lane's stream: the other stream has not seen it (later rounds: fixed on sg itself)
    if (round == 1) RET(c->fork(c->stream(), sg));
    launch_fold_round_g(c->dcrt, a, partial, gtmp, sg);
    hipEvent_t g_ready = nullptr;   // the GEMM chain's last kernel waits for the G part
    if (sg != c->stream() && !(g_ready = c->join_mark(sg))) return LF_ERR_HIP;
    const u64 *Ei = nullptr;
    size_t ldE = 0;
    Fq3Const w01[2] = {};
    if (sv_split) {
        // (every GEMM round so far ran in order: rounds 1..round-1 are all GEMM rounds when this one is, their challenges are pt[0..round-2])
        const Fq3 ci = lfs::eq_prefix(hv, beta.data(), pt.data(), round), bi = beta[round - 1];
        w01[0] = f3c(hv.ext_mul(ci, fq3_sub(fq3_one(), bi)));
        w01[1] = f3c(hv.ext_mul(ci, bi));
        svE_ensure(round);
        Ei = svE[round - 1]; ldE = m >> round;   // entries of E_round
    }
    const int rc = launch_sv_round(c->dcrt, svV, sv_bits[0], sv_bits[1], N, a.eqB, a.ld, a.p0, a.pcnt, K, d_mu, d_coef, sveb, svpart, svtot, svtp, gtmp, od, c->stream(),
                                   g_ready, Ei, ldE, w01);
    if (rc < 0) return i8_rc(rc);
    c->sv_round_mask |= 1u << (round - 1);
    return LF_OK;
}
// the kernel(s) of this round: its message (or, split, its three sums and the G part) goes to od
int FoldB2::dispatch(u32 round) {
    const int32_t *pL = S[0].planes, *pR = S[1].planes;
    hipStream_t st = c->stream();
    if (use_sv && (int)round <= c->tn.sv_rounds && round <= 3 && a.pcnt >= c->tn.sv_min && sv_shape_ok(1 << (round - 1), a.pcnt, K) && (a.p0 * ((size_t)1 << (round - 1))) % 256 == 0)
        return gemm_round(round);
    if ((round == 2 || (round == 1 && c->tn.fold_tab_r1)) && a.pcnt >= c->tn.tab_min) {   // (tab_min pairs; rounds 1-2 as table look-ups above this)
        std::vector<u64> poly;
        fold_tab_poly(hv, round, round == 2 ? pt[0] : fq3_zero(), poly);
        u64 *d_poly, *d_tp;
        RET(c->tbuf("fold_poly", 81 * 12 + 8, &d_poly));
        RET(c->tbuf("fold_tp", (size_t)K2 * 3 * 81 * 12, &d_tp));
        RET(c->h2d_small(d_poly, poly.data(), poly.size() * 8));
        launch_fold_round_tab(c->dcrt, (int)round, a, pL, pR, N, K, d_mu, d_poly, d_tp, partial, od, st);
        return LF_OK;
    }
    if (round == 1) launch_fold_round1(c->dcrt, a, pL, pR, N, K, d_mu, partial, od, st);
    else if (round == 2) launch_fold_round2(c->dcrt, a, pL, pR, N, K, d_mu, f3c(pt[0]), partial, od, st);
    else if (fmode == 3 && c->dcrt.nu2p40) {
        u64 *mutab;
        RET(c->tbuf("fold_mutab", (size_t)3 * K2 * 3 * 81 * 4, &mutab));
        launch_fold_round_lut_mu(c->dcrt, a, pL, pR, N, d_lut, mutab, K, d_mu, partial, od, st);
    } else if (fmode == 3) launch_fold_round_lut(c->dcrt, a, pL, pR, N, d_lut, K, d_mu, partial, od, st);
    else if (fmode == 4 && use_r4tab) {
        u64 *r4sq, *r4mt;
        RET(c->tbuf("fold_r4sq", (size_t)6561 * 4, &r4sq));
        RET(c->tbuf("fold_r4mt", (size_t)K2 * 3 * 162 * 4, &r4mt));
        launch_fold_round_lut_fix_tab(c->dcrt, a, pL, pR, N, d_lut, f3c(pt[round - 2]), r4sq, r4mt, use_r5 ? nullptr : (u64 *)curF, ldF, K, d_mu, partial, od, st, Er, ldEr);
    } else if (fmode == 7) {
        u64 *r5xx, *r5yy, *r5mt;
        RET(c->tbuf("fold_r5xx", (size_t)6561 * 4, &r5xx));
        RET(c->tbuf("fold_r5yy", (size_t)6561 * 4, &r5yy));
        RET(c->tbuf("fold_r5mt", (size_t)K2 * 3 * 324 * 4, &r5mt));
        launch_fold_round_lut_fix5(c->dcrt, a, pL, pR, N, d_lut, f3c(pt[round - 3]), f3c(pt[round - 2]), r5xx, r5yy, r5mt, (u64 *)curF, ldF, K, d_mu, partial, od, st, Er, ldEr);
    } else if (fmode == 4) launch_fold_round_lut_fix(c->dcrt, a, pL, pR, N, d_lut, f3c(pt[round - 2]), (u64 *)curF, ldF, K, d_mu, partial, od, st);
    else if (fmode == 1) launch_fold_round_fix(c->dcrt, a, prevF, prevld, f3c(pt[round - 2]), (u64 *)curF, ldF, K, d_mu, partial, od, st, Er, ldEr);
    else launch_fold_round(c->dcrt, a, curF, ldF, K, d_mu, partial, od, st);
    if (split_now) {   // the G part of the message (eqL G1 + eqR G2 at X = 0..4) from its own kernel, behind the three sums of the table kernel
        u64 *partial_g;
        RET(c->tbuf("round_partial_g", round_partial_words(), &partial_g));
        launch_fold_round_g(c->dcrt, a, partial_g, od + 120, st);
    }
    return LF_OK;
}
// the message in mapped host memory (od_host).  Sharded step: partial message in device memory -> all-gather + modular sum in stream -> host
int FoldB2::collect(u32 round) {
    if (od == od_shard) {
        if (sharded) RET(exchange_modsum_dev(c, od, (size_t)(deg + 1) * 24));
        HIPCHK(hipMemcpyAsync(od_host, od, (size_t)(deg + 1) * 24 * 8, hipMemcpyDeviceToHost, c->stream()));
    }
    return c->lane_sync();
}
int FoldB2::rounds() {
    size_t ph = c->ev_begin(14);
    { HostTimer ht(c); lfs::sumcheck_prologue<GoldV>(tr, P.s, deg); }
    RET(rounds_begin());
    for (u32 round = 1; round <= P.s; round++) {
        fmode = 0;
        bool done = false;
        RET(tail_handoff(round, &done));
        if (done) break;
        if (round > 1) {
            const size_t nn = a.n / 2;
            u64 *dst = T5[flip];
            bool gathered = false;
            RET(fix_tables(round, dst, &gathered));
            if (!gathered) RET(choose_producer(round));
            set_tables(dst, nn);
            flip ^= 1;
        }
        if (sharded && !shard_keep(c, 1, a.n)) sharded = false;   // (round 1 of a tiny instance)
        if (sharded) { a.pcnt = a.n / 2 / Gw; a.p0 = gr * a.pcnt; a.pF0 = a.p0; }
        else { a.p0 = 0; a.pcnt = a.n / 2; a.pF0 = 0; }
        decide_split(round);
        size_t ev = c->ev_begin(0);
        RET(dispatch(round));
        c->ev_end(ev);
        LF_TRACE(c, "fold round");
        RET(collect(round));
        u64 *evs = msg(round);
        if (split_now) {   // od_host[e][slot], e = 0..2: the sums A_e = sum_p E[p] Q_e(p); od_host[120 + X * 24 + ..]: the G part at X = 0..4
            HostTimer ht2(c);
            lfs::complete_fold_split(hv, sp, od_host, od_host + 120, msg(round - 1), pt[round - 2], evs);
        } else
            memcpy(evs, od_host, (size_t)(deg + 1) * 24 * 8);
        HostTimer ht(c);
        pt[round - 1] = lfs::sumcheck_round<GoldV>(tr, evs, deg + 1);
        if (round <= 3 || round == 6 || round == 10) TL_MARK_ROUND("  round", round);
    }
    TL_MARK(" fold sumcheck");
    c->ev_end(ph);
    return LF_OK;
}
int FoldB2::evaluations() {
    u64 *red;
    RET(c->tbuf("red_partial", 256 * 4096, &red));
    // the helper lane's stream is idle here: every second q_j is gathered there, and the eta products of the right side run there
    hipStream_t s1 = (t_lane == 0 && c->sh_world == 1 && c->st_lane[1]) ? c->st_lane[1] : c->stream();
    // q_j = M_j^T eq(r_o): one launch that leaves the packed digits both sides read (no words, no dec_q) where both sides' inner products take them; otherwise
    // the gathers into words, every second one on s1
    const bool fused_q = q_pack_takes(c, S[0].z, n, K) && q_pack_takes(c, S[1].z, n, K);
    unsigned char *ybq = nullptr;
    RET(eval_buffers(!fused_q));
    if (fused_q) RET(q_pack_dev(c, S[0].z, eq0, &ybq));
    else RET(gather_q(s1));
    // theta for both sides first, then eta; the host absorbs theta while the GPU still computes the eta dot products
    RET(c->pin((size_t)K2 * 72 + (size_t)K2 * P.t * 24));
    u64 *hp = c->h_pin_ref();
    // theta = f-hat_{k,d}(r_o): the f-hat tables of the sumcheck, fixed at r_1..r_{s-1}, have two entries left, so one more fix gives
    // the evaluations evaluate_mles would recompute from the witness (exact arithmetic: the same words).  Instances with fewer than
    // 4 variables never materialise the tables, and LF_THETA_EVAL=1 keeps the stand-alone evaluation (masked +-eq sums).
    if (P.s >= 4 && curF && ldF == 2 && !c->tn.theta_eval) launch_fix_final(c->dcrt, curF, K2 * 3 * 8, f3c(pt[P.s - 1]), d_theta, c->stream());
    else {
        size_t i0, cnt;
        shard_slice(c, N, &i0, &cnt);
        for (int sd = 0; sd < 2; sd++) RET(coef_eval_dev(c, S[sd].planes + i0, cnt, eq0 + i0, m, K, 1, red, d_theta + (size_t)sd * K * 72, N));
        RET(exchange_modsum_dev(c, d_theta, (size_t)K2 * 72));
    }
    HIPCHK(hipMemcpyAsync(hp, d_theta, (size_t)K2 * 72 * 8, hipMemcpyDeviceToHost, c->stream()));
    if (!c->ev_theta) HIPCHK(hipEventCreateWithFlags(&c->ev_theta, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_theta, c->stream()));
    {
        size_t c0, cnt;
        shard_slice(c, n, &c0, &cnt);
        // the two sides stream their own 0.8 GB of z_k: side by side on the two streams
        if (s1 != c->stream()) {
            // the digits of q are the same for both sides: packed once, before the streams part
            if (!fused_q && !c->tn.dot_valu && cnt >= c->tn.dot_min && P.t <= 3 && K <= 16 && ((((size_t)(S[0].z + c0)) ^ ((size_t)(S[1].z + c0))) & 15) == 0) {
                RET(c->tbuf("dot_yb", dot_i8_yb_bytes(n + 1), &ybq));
                const int rc = launch_dot_pack_y(S[0].z + c0, q + c0, n, P.t, cnt, ybq, c->stream());
                if (rc == i8mma::I8_ERR_HIP) return LF_ERR_HIP;
                if (rc < 0) ybq = nullptr;
            }
            RET(c->fork(c->stream(), s1));           // q = M_j^T eq(r_o) is ready (and packed)
            u64 *dpart1;
            RET(c->tbuf("dot_partial1", dot_partial_words(K, P.t), &dpart1));
            RET(dot_batch_dev(c, S[1].z + c0, n, K, q + c0, n, P.t, cnt, dpart1, d_eta + (size_t)K * P.t * 24, s1, "_1", ybq));
            if (!c->join_mark(s1)) return LF_ERR_HIP;
            RET(dot_batch_dev(c, S[0].z + c0, n, K, q + c0, n, P.t, cnt, dpart, d_eta, nullptr, "", ybq));
            RET(c->join_wait(c->stream()));
        } else
            for (int sd = 0; sd < 2; sd++) RET(dot_batch_dev(c, S[sd].z + c0, n, K, q + c0, n, P.t, cnt, dpart, d_eta + (size_t)sd * K * P.t * 24, nullptr, "", ybq));
        RET(exchange_modsum_dev(c, d_eta, (size_t)K2 * P.t * 24));
    }
    HIPCHK(hipMemcpyAsync(hp + (size_t)K2 * 72, d_eta, (size_t)K2 * P.t * 24 * 8, hipMemcpyDeviceToHost, c->stream()));
    HIPCHK(hipEventSynchronize(c->ev_theta));
    memcpy(theta(), hp, (size_t)K2 * 72 * 8);
    {
        HostTimer ht(c);
        tr.absorb_ring(theta(), (size_t)K2 * 3);
    }
    HIPCHK(hipStreamSynchronize(c->stream()));
    memcpy(eta(), hp + (size_t)K2 * 72, (size_t)K2 * P.t * 24 * 8);
    TL_MARK(" theta/eta");
    return LF_OK;
}
int fold_impl(lf_ctx *c, Transcript &tr, SideState *S /* [2] */, u64 *lcccs_out, lf_witness **w_out, u64 *proof) {
    if (c->P.b != 2) return fold_impl_sb(c, tr, S, lcccs_out, w_out, proof);   // small-base path (lf_fold_sb.cpp)
    FoldB2 f(c, tr, S, proof);
    RET(f.prepare());
    RET(f.rounds());
    size_t ph = c->ev_begin(15);
    RET(f.evaluations());
    RET(f.finish(lcccs_out, w_out, [&](const std::vector<int8_t> &rho8, int8_t *d_rho, int32_t *npl) -> int {
        HIPCHK(hipMemcpyAsync(d_rho, rho8.data(), rho8.size(), hipMemcpyHostToDevice, c->stream()));
        LF_TRACE(c, "theta/eta");
        int rc = i8mma::I8_ERR_SHAPE;
        if (!c->tn.fold_witness_valu) {
            int rho_max = 0;
            for (int8_t r : rho8) rho_max = std::max(rho_max, std::abs((int)r));
            rc = launch_fold_witness_i8(S[0].planes, S[1].planes, f.N, f.K, d_rho, rho_max, npl, c->stream());
        }
        if (rc == i8mma::I8_ERR_SHAPE) launch_fold_witness(S[0].planes, S[1].planes, f.N, f.K, d_rho, npl, c->stream());   // (the shapes the int8 form declines, or the switch)
        return rc == i8mma::I8_ERR_HIP ? LF_ERR_HIP : LF_OK;
    }));
    c->ev_end(ph);
    return LF_OK;
}

// ---- generic linearization-shaped sumcheck through the ABI (tests / SURVEY 8b) -------------------------------------------------
static int sumcheck_lin_begin_api(lf_ctx *c, const uint64_t *tables, const uint64_t *eq_point, Origin org) {
    if (LF_XB(c) && tables && eq_point && c->have_ccs_any()) { XB x(c, true); const lf_params &P = c->params_any(); return sumcheck_lin_begin_api(c, tables, x.ext_in(eq_point, P.s), org); }
    if (!c || !tables || !eq_point) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::sumcheck_lin_begin(c->bb->p, tables, eq_point, org) : ring_ops<GoldRing>::sumcheck_lin_begin(c, tables, eq_point, org);
}
int lf_sumcheck_lin_begin(lf_ctx *c, const uint64_t *tables, const uint64_t *eq_point) { return sumcheck_lin_begin_api(c, tables, eq_point, Origin::host); }
int lf_sumcheck_lin_begin_dev(lf_ctx *c, const uint64_t *tables, const uint64_t *eq_point) { return sumcheck_lin_begin_api(c, tables, eq_point, Origin::device); }
int lf_sumcheck_lin_round(lf_ctx *c, const uint64_t *r_prev, uint64_t *evals_out) {
    if (LF_XB(c) && evals_out) { XB x(c); int rc = lf_sumcheck_lin_round(c, x.ext_in(r_prev, 1), evals_out); if (rc == LF_OK) x.ring_out(evals_out, c->params_any().d + 2); return rc; }
    if (!c || !evals_out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::sumcheck_lin_round(c->bb->p, r_prev, evals_out) : ring_ops<GoldRing>::sumcheck_lin_round(c, r_prev, evals_out);
}
int lf_sumcheck_lin_end(lf_ctx *c) {
    if (!c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::sumcheck_lin_end(c->bb->p) : ring_ops<GoldRing>::sumcheck_lin_end(c);
}

// ---- the generic sumcheck (include/lfhip_sumcheck.h): argument checks and ring dispatch; bodies in lf_ring_host.h (mlsumcheck_*), kernel lf_mlsumcheck.hip ----
static int mlsumcheck_begin_api(lf_ctx *c, const lf_vpoly *vp, const uint64_t *tables, Origin org) {
    if (!c || !vp || !tables || !vp->term_off || !vp->term_idx || !vp->coef) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::mlsumcheck_begin(c->bb->p, vp, tables, org) : ring_ops<GoldRing>::mlsumcheck_begin(c, vp, tables, org);
}
int lf_mlsumcheck_begin(lf_ctx *c, const lf_vpoly *vp, const uint64_t *tables) { return mlsumcheck_begin_api(c, vp, tables, Origin::host); }
int lf_mlsumcheck_begin_device(lf_ctx *c, const lf_vpoly *vp, const uint64_t *tables) { return mlsumcheck_begin_api(c, vp, tables, Origin::device); }
int lf_mlsumcheck_round(lf_ctx *c, const uint64_t *r_prev, uint64_t *evals_out) {
    if (!c || !evals_out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::mlsumcheck_round(c->bb->p, r_prev, evals_out) : ring_ops<GoldRing>::mlsumcheck_round(c, r_prev, evals_out);
}
int lf_mlsumcheck_final(lf_ctx *c, const uint64_t *r_last, uint64_t *evals_out) {
    if (!c || !r_last || !evals_out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::mlsumcheck_final(c->bb->p, r_last, evals_out) : ring_ops<GoldRing>::mlsumcheck_final(c, r_last, evals_out);
}
int lf_mlsumcheck_end(lf_ctx *c) {
    if (!c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::mlsumcheck_end(c->bb->p) : ring_ops<GoldRing>::mlsumcheck_end(c);
}
// MLSumcheck::prove_as_subprotocol: the round loop with the transcript is ring_ops::mlsumcheck_prove, one body over the split form for both origins
static int mlsumcheck_prove_api(lf_ctx *c, lf_transcript *t, const lf_vpoly *vp, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out, uint64_t *final_out,
                                Origin org) {
    if (!c || !t || !vp || !tables || !msgs_out || !point_out || !vp->term_off || !vp->term_idx || !vp->coef || (c->bb != nullptr) != (t->bb != nullptr))
        return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::mlsumcheck_prove(c->bb->p, *t->bb, vp, tables, msgs_out, point_out, final_out, org)
                 : ring_ops<GoldRing>::mlsumcheck_prove(c, t->t, vp, tables, msgs_out, point_out, final_out, org);
}
int lf_mlsumcheck_prove(lf_ctx *c, lf_transcript *t, const lf_vpoly *vp, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out, uint64_t *final_out) {
    return mlsumcheck_prove_api(c, t, vp, tables, msgs_out, point_out, final_out, Origin::host);
}
int lf_mlsumcheck_prove_device(lf_ctx *c, lf_transcript *t, const lf_vpoly *vp, const uint64_t *tables, uint64_t *msgs_out, uint64_t *point_out,
                               uint64_t *final_out) {
    return mlsumcheck_prove_api(c, t, vp, tables, msgs_out, point_out, final_out, Origin::device);
}

// PoseidonSponge on the device: a script of absorb / squeeze operations on a fresh sponge, one wave.  ops[i] =
// (kind << 24) | count: kind 0 absorbs the next `count` words of absorb_words, kind 1 squeezes `count` words into squeezed_out.
// state_out (optional, 26 words): the 24 state words, the rate index and the mode (1 = squeezing) afterwards.
int lf_device_sponge(lf_ctx *c, const uint32_t *ops, size_t nops, const uint64_t *absorb_words, size_t n_words, uint64_t *squeezed_out,
                     size_t n_out, uint64_t *state_out) {
    if (!c || !ops || !nops || (!absorb_words && n_words) || (!squeezed_out && n_out)) return LF_ERR_INVALID;
    if (c->bb) return LF_ERR_UNSUPPORTED;   // the BabyBear transcript stays on the host
    size_t na = 0, ns = 0;
    for (size_t i = 0; i < nops; i++) {
        if ((ops[i] >> 24) > 1) return LF_ERR_INVALID;
        ((ops[i] >> 24) ? ns : na) += ops[i] & 0xffffff;
    }
    if (na != n_words || ns != n_out) return LF_ERR_INVALID;
    for (size_t i = 0; i < n_words; i++)
        if (absorb_words[i] >= LF_P) return LF_ERR_INVALID;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    RET(c->poseidon_setup());
    u64 *dw, *dout;
    u32 *dops;
    RET(c->tbuf("sp_words", n_words + 8, &dw));
    RET(c->tbuf("sp_out", n_out + 32, &dout));
    RET(c->tbuf("sp_ops", nops + 8, &dops));
    if (n_words) HIPCHK(hipMemcpyAsync(dw, absorb_words, n_words * 8, hipMemcpyHostToDevice, c->stream()));
    HIPCHK(hipMemcpyAsync(dops, ops, nops * 4, hipMemcpyHostToDevice, c->stream()));
    launch_sponge_script(c->d_poseidon, c->d_poseidon + 720, dops, (u32)nops, dw, dout, dout + n_out, c->stream());
    std::vector<u64> h(n_out + 26);
    HIPCHK(hipMemcpyAsync(h.data(), dout, (n_out + 26) * 8, hipMemcpyDeviceToHost, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));
    if (n_out) memcpy(squeezed_out, h.data(), n_out * 8);
    if (state_out) memcpy(state_out, h.data() + n_out, 26 * 8);
    return LF_OK;
}

// ---- the folding sumcheck through the ABI: the bodies and the layout of `tables` are in lf_ring_host.h (ring_ops::sumcheck_fold_*)
static int sumcheck_fold_begin_api(lf_ctx *c, const uint64_t *tables, const uint64_t *mu, Origin org) {
    if (LF_XB(c) && tables && mu && c->have_ccs_any()) { XB x(c, true); const lf_params &P = c->params_any(); return sumcheck_fold_begin_api(c, tables, x.ext_in(mu, 2 * P.K), org); }
    if (!c || !tables || !mu) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::sumcheck_fold_begin(c->bb->p, tables, mu, org) : ring_ops<GoldRing>::sumcheck_fold_begin(c, tables, mu, org);
}
int lf_sumcheck_fold_begin(lf_ctx *c, const uint64_t *tables, const uint64_t *mu) { return sumcheck_fold_begin_api(c, tables, mu, Origin::host); }
int lf_sumcheck_fold_begin_dev(lf_ctx *c, const uint64_t *tables, const uint64_t *mu) { return sumcheck_fold_begin_api(c, tables, mu, Origin::device); }
int lf_sumcheck_fold_round(lf_ctx *c, const uint64_t *r_prev, uint64_t *evals_out) {
    if (LF_XB(c) && evals_out) { XB x(c); int rc = lf_sumcheck_fold_round(c, x.ext_in(r_prev, 1), evals_out); if (rc == LF_OK) x.ring_out(evals_out, 2 * c->params_any().b + 1); return rc; }
    if (!c || !evals_out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::sumcheck_fold_round(c->bb->p, r_prev, evals_out) : ring_ops<GoldRing>::sumcheck_fold_round(c, r_prev, evals_out);
}
int lf_sumcheck_fold_end(lf_ctx *c) {
    if (!c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::sumcheck_fold_end(c->bb->p) : ring_ops<GoldRing>::sumcheck_fold_end(c);
}

// compute_f_0 (nifs/folding.rs:258-268): out[j] = sum_i coef_i (.) tables_i[j] with ring-element coefficients (8 distinct slots)
static int lincomb_api(lf_ctx *c, const uint64_t *coef, const uint64_t *tables, size_t n_terms, size_t len, uint64_t *out, Origin org) {
    if (LF_XB(c) && coef && tables && out) { XB x(c, true); return lincomb_api(c, x.ring_in(coef, n_terms), tables, n_terms, len, out, org); }
    if (!c || !coef || !tables || !out || !n_terms || !len) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::lincomb(c->bb->p, coef, tables, n_terms, len, out, org) : ring_ops<GoldRing>::lincomb(c, coef, tables, n_terms, len, out, org);
}
int lf_lincomb(lf_ctx *c, const uint64_t *coef, const uint64_t *tables, size_t n_terms, size_t len, uint64_t *out) {
    return lincomb_api(c, coef, tables, n_terms, len, out, Origin::host);
}
int lf_lincomb_dev(lf_ctx *c, const uint64_t *coef, const uint64_t *tables, size_t n_terms, size_t len, uint64_t *out) {
    return lincomb_api(c, coef, tables, n_terms, len, out, Origin::device);
}
// calculate_challenged_mz_mle (nifs/folding.rs:208-226) and the f-hat half of prepare_g1_and_3_k_mles_list (folding/utils.rs:524-546):
// out[x] = sum_{i<groups} sum_{j<per_group} c_i^{j+1} T_{i,j}[x] (the reference's Horner loop `mle += M; mle *= c_i` over j reversed)
static int horner_combine_api(lf_ctx *c, const uint64_t *tables, size_t groups, size_t per_group, size_t len, const uint64_t *challenges, uint64_t *out, Origin org) {
    if (LF_XB(c) && tables && challenges && out) { XB x(c, true); return horner_combine_api(c, tables, groups, per_group, len, x.ext_in(challenges, groups), out, org); }
    if (!c || !tables || !challenges || !out || !groups || !per_group || !len) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::horner_combine(c->bb->p, tables, groups, per_group, len, challenges, out, org)
                 : ring_ops<GoldRing>::horner_combine(c, tables, groups, per_group, len, challenges, out, org);
}
int lf_horner_combine(lf_ctx *c, const uint64_t *tables, size_t groups, size_t per_group, size_t len, const uint64_t *challenges, uint64_t *out) {
    return horner_combine_api(c, tables, groups, per_group, len, challenges, out, Origin::host);
}
int lf_horner_combine_dev(lf_ctx *c, const uint64_t *tables, size_t groups, size_t per_group, size_t len, const uint64_t *challenges, uint64_t *out) {
    return horner_combine_api(c, tables, groups, per_group, len, challenges, out, Origin::device);
}

