"""Goldilocks device arithmetic at its reduction corners, bit-exact against big integers.

The parity tests feed the kernels pseudo-random residues, which never take the rare branches of lf_field.cuh (the borrow and the hl == 0 case of
fq_reduce128_loose, loose results in [p, 2^64), either wrap of fq_from_s128).  Every case here goes through an existing entry point with operands from the
reduction-corner grid of tests/field_corners.py and is compared word for word with that module's reference on Python ints (`%`), which is independent of
lf_field.cuh and of the oracle's fast reduction.  tests/test_field_corners_cpu.py pins the reference against the oracle on the same tables and proves that
each case's products reach every corner.  The folding sumcheck, which the big-integer code does not restate, is compared with the oracle."""
import numpy as np
import pytest

import field_corners as fc
import lfo
from latticefold_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs():
    """references computed once and shared"""
    return {}


def _ctx(generic=False):
    c = api.Context(0)
    if generic:
        nu2, y2 = fc.other_nonresidue()
        c.set_ring_tables(nu2, y2)
    return c


def _ref(generic):
    return fc.Ref(nu=fc.other_nonresidue()[0]) if generic else fc.Ref()


def _same(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: device {int(np.asarray(got)[tuple(bad[0])]):#x}, reference {int(np.asarray(want)[tuple(bad[0])]):#x}"


# ---- products: fq3_mul_2p40 / fq3_mul<false> on the device's multiply path, grid x grid in every coordinate position ----------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["nu2p40", "generic"])
@pytest.mark.parametrize("kind", fc.PRODUCT_KINDS)
def test_products(kind, generic):
    wl, z = fc.products_case(kind)
    ref = _ref(generic)
    want = fc.pack(ref.spmv(wl.rowptr[0], wl.col[0], fc.elems(wl.val[0]), fc.elems(z), wl.m))
    ctx = _ctx(generic)
    try:
        ctx.load_ccs(wl)
        _same(ctx.mat_vec_mul(0, z), want, f"mat_vec_mul/{kind}")
    finally:
        ctx.close()


# ---- eq tables and MLE evaluations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["nu2p40", "generic"])
@pytest.mark.parametrize("nv", fc.EQ_NVS)
def test_build_eq_and_evaluate_mles(nv, generic):
    ref = _ref(generic)
    ctx = _ctx(generic)
    try:
        for pk in fc.EQ_POINTS:
            pt = fc.point(pk, nv)
            _same(ctx.build_eq(pt), np.array(ref.eq_table(fc.exts(pt)), dtype=np.uint64), f"build_eq/nv{nv}/{pk}")
            for ln in sorted({1 << nv, max(1, (1 << nv) - 3)}):
                tabs = fc.mle_tables(nv, ln)
                want = fc.pack([ref.mle_eval(fc.elems(t), fc.exts(pt)) for t in tabs])
                _same(ctx.evaluate_mles(tabs, pt), want, f"evaluate_mles/nv{nv}/{pk}/len{ln}")
    finally:
        ctx.close()


# ---- lincomb / horner_combine at the group counts of a fold step with K = 4 and K = 8 ---------------------------------------------------------------
@pytest.mark.parametrize("K,ln", fc.COMBINE_CASES)
def test_lincomb_and_horner_combine(K, ln):
    ref = fc.Ref()
    ctx = _ctx()
    try:
        coef, tabs = fc.lincomb_case(K, ln)
        _same(api.lincomb(ctx, coef, tabs), fc.pack(ref.lincomb(fc.elems(coef), fc.elems(tabs))), f"lincomb/K{K}")
        tabs, ch = fc.horner_case(K, ln)
        _same(api.horner_combine(ctx, tabs, ch), fc.pack(ref.horner_combine(fc.elems(tabs), fc.exts(ch))), f"horner_combine/K{K}")
    finally:
        ctx.close()


# ---- the linearization sumcheck, every round message ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ccs,kind,generic", [c + (False,) for c in fc.LIN_CASES] + [("r1cs", "corner", True)])
def test_sumcheck_lin_round_messages(ccs, kind, generic):
    wl, tabs, beta, ch = fc.lin_case(ccs, kind)
    ref = _ref(generic)
    want = fc.pack(ref.lin_rounds(fc.elems(tabs), fc.exts(beta), wl.S_off, wl.S_idx, fc.elems(wl.c), wl.d, fc.exts(ch)))
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


@pytest.mark.parametrize("env", [{}, {"LF_LIN_SPLIT_MIN": "16", "LF_NO_TAIL": "1"}], ids=["default", "split"])
@pytest.mark.parametrize("ccs", ["r1cs", "deg3"])
def test_linearization_of_a_corner_witness(ccs, env, monkeypatch):
    """the round kernels of the prover itself -- the lazy split-eq rounds and the plain ones (LF_LIN_SPLIT_MIN=16, LF_NO_TAIL=1), the persistent tail by default --
    on tables M_j z of a witness drawn from the grid.  The challenges come from the transcript here, so the reference is the oracle's linearization."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wl = fc.lin_witness_case(ccs)
    inst = lfo.Instance(wl)
    ctx = _ctx()
    try:
        ctx.load_ccs(wl)
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=wl.ajtai_matrix())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        f = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        acc_g, lin_g = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
        acc_o, lin_o = inst.linearize(lfo.Transcript(), cccs, f)
        assert ctx.lin_split_rounds() == (wl.s - 3 if env else 0)
        _same(lin_g, lin_o, f"linearization proof/{ccs}")
        _same(acc_g, acc_o, f"lcccs/{ccs}")
    finally:
        ctx.close()


# ---- the folding sumcheck (b = 2 and b = 4) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", fc.FOLD_CASES)
def test_sumcheck_fold_round_messages(name, kind):
    wl, tabs, mu = fc.fold_case(name, kind)
    ref = fc.Ref()
    for idx, pt in zip((0, 2, 4), fc.fold_eq_points(wl, kind)):
        tabs[idx] = np.tile(np.array(ref.eq_table(fc.exts(pt)), dtype=np.uint64), (1, 8))
    inst = lfo.Instance(wl)
    msgs_o, pt_o = inst.sumcheck_fold(lfo.Transcript(), tabs, fc.embed(mu))
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


# ---- CRT / ICRT: 24-term row sums on the Acc path with its carry counter ----------------------------------------------------------------------------
def test_crt_icrt():
    """against the 24 x 24 matrices on Python ints (fc.crt_matrices); one case over all kinds of rows, which together reach the corners of the Acc path"""
    F, I = fc.crt_matrices()
    ctx = _ctx()
    try:
        for kind in fc.CRT_ROWS:
            for count in (1, 7, 257):
                x = fc.crt_rows(kind, count)
                g = ctx.crt(x)
                _same(g, fc.matvec(F, x), f"crt/{kind}/{count}")
                _same(ctx.icrt(x), fc.matvec(I, x), f"icrt/{kind}/{count}")
                _same(ctx.icrt(g), x, f"icrt(crt)/{kind}/{count}")
    finally:
        ctx.close()


def test_selftest_field_on_corner_operands():
    """lf_selftest_field: the device computes, the host compares with unsigned __int128 %; the first 1452 operand pairs are the grid pairs (n below and above that)"""
    ctx = _ctx()
    try:
        for seed, n in ((1, 1), (2, 255), (3, 1452), (4, 5000)):
            assert ctx.selftest_field(seed, n) == 0
    finally:
        ctx.close()
