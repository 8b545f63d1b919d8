"""BabyBear device arithmetic at the extremes of its Montgomery words, word for word against big integers.

The BabyBear kernels work on centred Montgomery words in [-H, H] (bb_field.cuh), and their bounds -- nine products in one signed 64-bit column, mred's
pre-centring of the high half, the 96-bit lazy sums, the balanced base-256 digits of the int8 paths -- are bounds on that word.  Canonical corners (p - 1,
(p +- 1) / 2) are words at 27 % and 13 % of H and reach none of them.  Every case here goes through an existing entry point with operands from the DEVICE-WORD
grid of tests/field_corners.py (EDGE_BW, the saturating pairs, tables of +-H) and is compared with that module's reference on Python ints (`%`), which knows
nothing of Montgomery form.  tests/test_bb_field_corners_cpu.py pins the reference against the oracle on the same tables and proves that each case's operands
reach the branches.  The folding sumcheck and the decomposition, which the big-integer code does not restate, are compared with the oracle."""
import numpy as np
import pytest

import field_corners as fc
import lfo_bb
from field_corners import BB
from latticefold_amd import api

pytestmark = pytest.mark.gpu


def _ctx(generic=False):
    c = api.Context(0, ring=BB)
    if generic:
        nu2, y2 = fc.other_nonresidue_bb()
        c.set_ring_tables(nu2, y2)
    return c


def _ref(generic):
    return fc.Ref(BB, nu=fc.other_nonresidue_bb()[0]) if generic else fc.Ref(BB)


def _same(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: device {int(np.asarray(got)[tuple(bad[0])]):#x}, reference {int(np.asarray(want)[tuple(bad[0])]):#x}"


# ---- products: e9_mul on the device's multiply path, word grid x word grid in every coordinate position behind the saturating pairs --------------------
@pytest.mark.parametrize("generic", [False, True], ids=["nu2", "generic"])
@pytest.mark.parametrize("kind", fc.PRODUCT_KINDS)
def test_products(kind, generic):
    wl, z = fc.products_case_bb(kind)
    ref = _ref(generic)
    want = fc.pack(ref.spmv(wl.rowptr[0], wl.col[0], fc.elems(wl.val[0], BB), fc.elems(z, BB), wl.m))
    ctx = _ctx(generic)
    try:
        ctx.load_ccs(wl)
        _same(ctx.mat_vec_mul(0, z), want, f"mat_vec_mul/{kind}")
    finally:
        ctx.close()


# ---- eq tables and MLE evaluations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["nu2", "generic"])
@pytest.mark.parametrize("nv", fc.EQ_NVS)
def test_build_eq_and_evaluate_mles(nv, generic):
    ref = _ref(generic)
    ctx = _ctx(generic)
    try:
        for pk in fc.EQ_POINTS_BB:
            pt = fc.point(pk, nv, BB, words=True)
            _same(ctx.build_eq(pt), np.array(ref.eq_table(fc.exts(pt)), dtype=np.uint64), f"build_eq/nv{nv}/{pk}")
            for ln in sorted({1 << nv, max(1, (1 << nv) - 3)}):
                tabs = fc.mle_tables_bb(nv, ln)
                want = fc.pack([ref.mle_eval(fc.elems(t, BB), fc.exts(pt)) for t in tabs])
                _same(ctx.evaluate_mles(tabs, pt), want, f"evaluate_mles/nv{nv}/{pk}/len{ln}")
    finally:
        ctx.close()


# ---- lincomb / horner_combine: 2K resp. 6K un-reduced products in one 96-bit sum -----------------------------------------------------------------
@pytest.mark.parametrize("K,ln", fc.COMBINE_CASES)
def test_lincomb_and_horner_combine(K, ln):
    ref = fc.Ref(BB)
    ctx = _ctx()
    try:
        for kind in fc.COMBINE_KINDS_BB:
            coef, tabs = fc.lincomb_case_bb(K, ln, kind)
            _same(api.lincomb(ctx, coef, tabs), fc.pack(ref.lincomb(fc.elems(coef, BB), fc.elems(tabs, BB))), f"lincomb/K{K}/{kind}")
            tabs, ch = fc.horner_case_bb(K, ln, kind)
            _same(api.horner_combine(ctx, tabs, ch), fc.pack(ref.horner_combine(fc.elems(tabs, BB), fc.exts(ch))), f"horner_combine/K{K}/{kind}")
    finally:
        ctx.close()


# ---- the linearization sumcheck, every round message ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ccs,kind,generic", [c + (False,) for c in fc.LIN_CASES_BB] + [("r1cs", "corner", True)])
def test_sumcheck_lin_round_messages(ccs, kind, generic):
    wl, tabs, beta, ch = fc.lin_case_bb(ccs, kind)
    ref = _ref(generic)
    want = fc.pack(ref.lin_rounds(fc.elems(tabs, BB), fc.exts(beta), wl.S_off, wl.S_idx, fc.elems(wl.c, BB), wl.d, fc.exts(ch)))
    ctx = _ctx(generic)
    try:
        ctx.load_ccs(wl)
        sc = api.MLSumcheckLin(ctx, tabs, beta)
        for rnd in range(wl.s):
            msg = sc.prove_round(None if rnd == 0 else ch[rnd - 1])
            _same(msg, want[rnd], f"lin/{ccs}/{kind} round {rnd + 1}")
        sc.end()
    finally:
        ctx.close()


# ---- the folding sumcheck ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", fc.FOLD_CASES_BB)
def test_sumcheck_fold_round_messages(name, kind):
    wl, tabs, mu = fc.fold_case_bb(name, kind)
    ref = fc.Ref(BB)
    for idx, pt in zip((0, 2, 4), fc.fold_eq_points_bb(wl, kind)):
        tabs[idx] = np.tile(np.array(ref.eq_table(fc.exts(pt)), dtype=np.uint64), (1, 8))
    inst = lfo_bb.Instance(wl)
    msgs_o, pt_o = inst.sumcheck_fold(lfo_bb.Transcript(), tabs, fc.embed(mu, BB))
    npts = 2 * wl.b + 1
    ctx = _ctx()
    try:
        ctx.load_ccs(wl)
        sc = api.MLSumcheckFold(ctx, tabs, mu)
        for rnd in range(wl.s):
            ev = sc.prove_round(None if rnd == 0 else pt_o[rnd - 1][:wl.tau])
            _same(ev, msgs_o[rnd * npts:(rnd + 1) * npts], f"fold/{name}/{kind} round {rnd + 1}")
        sc.end()
    finally:
        ctx.close()


# ---- CRT / ICRT ----------------------------------------------------------------------------------------------------------------------------------
def test_crt_icrt():
    """against the 72 x 72 matrices on Python ints (fc.crt_matrices_bb); rows of +-H, the rows that make every group of the dense inverse map as large as its
    matrix allows, and corner rows, at counts around the relayout tile of 64 elements"""
    F, I = fc.crt_matrices_bb()
    ctx = _ctx()
    try:
        for kind in fc.CRT_ROWS_BB:
            for count in fc.CRT_COUNTS_BB:
                x = fc.crt_rows_bb(kind, count, I)
                g = ctx.crt(x)
                _same(g, fc.matvec_bb(F, x), f"crt/{kind}/{count}")
                _same(ctx.icrt(x), fc.matvec_bb(I, x), f"icrt/{kind}/{count}")
                _same(ctx.icrt(g), x, f"icrt(crt)/{kind}/{count}")
    finally:
        ctx.close()


# ---- the int8 inner products and digit-plane evaluations, through the decomposition prover -------------------------------------------------------
def _decomposition(wl, r, monkeypatch, envs):
    """LFDecompositionProver.prove at the point r under each environment against the oracle's decomposition of the same LCCCS"""
    inst = lfo_bb.Instance(wl)
    f = inst.witness_from_w_ccs(wl.w_ccs)
    A = wl.ajtai_matrix()
    cccs = np.concatenate([lfo_bb.ajtai_commit(A, wl.kappa, wl.N, lfo_bb.crt(f)), wl.x_ccs])
    lc, _ = inst.linearize(lfo_bb.Transcript(), cccs, f)
    ctx = _ctx()
    try:
        ctx.load_ccs(wl)
        api.AjtaiCommitmentScheme(ctx, matrix=A)
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        for rr in r:
            lc = lc.copy()
            lc[:wl.s] = rr
            lcs_o, pr_o = inst.decomposition_prove(lfo_bb.Transcript(), A, lc, f)
            for env in envs:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                lcs_g, pr_g = api.LFDecompositionProver.prove(ctx, lc, wit, api.PoseidonTranscript(ring=BB))
                for k in env:
                    monkeypatch.delenv(k)
                K, t = wl.K, wl.t
                _same(pr_g[:K * t], pr_o[:K * t], f"u_s {env}")
                _same(pr_g[K * t:K * (t + 9)], pr_o[K * t:K * (t + 9)], f"v_s {env}")
                _same(pr_g, pr_o, f"decomposition proof {env}")
                _same(lcs_g, lcs_o, f"decomposed lcccs {env}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name,l", fc.DOT_SHAPES_BB)
def test_int8_inner_products_on_digit_boundary_words(name, l, monkeypatch):
    """k_dot_pack_y / k_bbdot_i8: r is a 0 / 1 point, so M_j^T eq(r) -- the Y operand -- is the dense row of fc.dot_case_bb: words with -128 and 127 at every
    digit position, +-H, runs of -0x3B808080; 192 columns (three steps of 64) and 130 (a partial last step).  Once on the matrix cores (LF_DOT_MIN lowers the
    driver's threshold of 4096 columns, as in test_fold_step_int8_inner_products_match_oracle) and once on the VALU kernel"""
    wl, r = fc.dot_case_bb(name, l)
    _decomposition(wl, [r], monkeypatch, [{"LF_DOT_MIN": "64"}, {"LF_DOT_MIN": "64", "LF_DOT_VALU": "1"}])


def test_int8_coefficient_evaluations_on_digit_boundary_words(monkeypatch):
    """k_bbce_i8 (v_s from the digit planes and eq): r = (x, 0, .., 0) makes 1 - x and x the two non-zero eq entries, x = canon(w) for digit-boundary words w"""
    from latticefold_amd.workload import make_workload
    wl = make_workload("B6")
    _decomposition(wl, [fc.ce_point(wl, w) for w in fc.CE_WORDS_BB], monkeypatch, [{}])


def test_selftest_field_on_word_grid_operands():
    """lf_selftest_field on this ring: the device computes, the host compares with %; the first fc.SELFTEST_PAIRS_BB operand pairs are the word-grid pairs and
    the saturating pairs (n below, at and above that), with nu = 2 and with the generic nu"""
    n0 = fc.SELFTEST_PAIRS_BB
    for generic in (False, True):
        ctx = _ctx(generic)
        try:
            for seed, n in ((1, 1), (2, 255), (3, n0 - 36), (4, n0 - 1), (5, n0), (6, n0 + 1), (7, 20000)):
                assert ctx.selftest_field(seed, n) == 0, (generic, seed, n)
        finally:
            ctx.close()
