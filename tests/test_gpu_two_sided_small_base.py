"""Decomposition bases b = 4, 8, 16 and wide constraint systems (Goldilocks, one GPU): fold steps of two DIFFERENT witnesses, word for word against the CPU
oracle's step for exactly that pair (tests/two_sided.py) -- the only two-witness comparison of the small-base path with the oracle.

Shapes: T8b4, T8b16 with every pair; T8b8, the ragged R61b4 / R61b16 (N = 244), (T8b4, K 9) and (T8b16, K 5) under digit rule 1, and O255b8 (N = 255 of
m = 256: the last pair of round 1 and of k_sb_materialize has one plane entry, the `2 p + 1 < n_planes` edge) with (base, chain1) and its swap.  Then a
three-step chain with a new witness per step, the sub-provers under one transcript with different sides, lf_sumcheck_fold_* on the device-built f-hat of the
parts of two different witnesses, and T8 / deg7 and T10 / mix8.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import fold_paths
import lfo
import two_sided
from latticefold_amd import api
from latticefold_amd.workload import P, chain_w_ccs, diag
from witness_parts_cases import oracle_parts
from witness_tables_ref import embed, fhat_np, rand_ring

pytestmark = pytest.mark.gpu
G = two_sided.G


@pytest.fixture(scope="module", autouse=True)
def _devices():
    yield
    two_sided.close_devices()


def _tr():
    return api.PoseidonTranscript()


@pytest.mark.parametrize("case", two_sided.SB_CASES, ids=two_sided.case_id)
def test_small_base_step_folds_two_witnesses_like_the_oracle(case, monkeypatch):
    ring, name, ccs, K, mode, pair = case
    c = two_sided.case(ring, name, pair, ccs, K, mode)
    assert c.wl.b != 2
    if name == "O255b8":
        assert c.wl.N == 255 and c.wl.m == 256
    two_sided.run_sets(c, fold_paths.SB_SETS, monkeypatch, fold_paths.expected, fold_paths.applied)


@pytest.mark.parametrize("case", two_sided.WIDE_CASES, ids=two_sided.case_id)
def test_wide_ccs_step_folds_two_witnesses_like_the_oracle(case, monkeypatch):
    ring, name, ccs, K, mode, pair = case
    c = two_sided.case(ring, name, pair, ccs, K, mode)
    assert c.wl.t > 4 and c.wl.d > 3
    two_sided.run_sets(c, fold_paths.SB_SETS, monkeypatch, fold_paths.expected, fold_paths.applied)


@pytest.mark.parametrize("name", ["T8b4", "T8b16"])
def test_three_step_chain_matches_the_oracle(name):
    """acc <- fold(acc, chain_w_ccs(wl, j)), j = 1, 2, 3: from step 2 on the left side is a folded witness, the right one a fresh one; the oracle runs along"""
    sh = two_sided.oracle_shape(two_sided.shape_key(G, name))
    dev = two_sided.case(G, name, ("base", "chain1")).dev
    wl, inst, ctx = sh.wl, sh.inst, dev.ctx
    base = dev.witness("base")
    acc, w_acc = base.acc, base.wit
    acc_o, f_acc = sh.side("base").acc, sh.side("base").f
    for j in range(1, 4):
        w = chain_w_ccs(wl, j)
        w_j = api.Witness.from_w_ccs(ctx, w)
        f_j = inst.witness_from_w_ccs(w)
        cccs_j = np.concatenate([lfo.ajtai_commit(sh.A, wl.kappa, wl.N, lfo.crt(f_j)), wl.x_ccs])
        assert (w_j.commit(dev.scheme) == cccs_j[:wl.kappa]).all(), (j, "cm")
        lc_o, f0_o, proof_o = inst.fold_step(lfo.Transcript(), sh.A, acc_o, f_acc, cccs_j, f_j)
        lc, w_next, proof = api.NIFSProver.prove(ctx, acc, w_acc, cccs_j, w_j, _tr())
        so, sg = two_sided.sections(wl, proof_o), two_sided.sections(wl, proof)
        bad = [k for k in so if not (so[k] == sg[k]).all()]
        assert not bad, (j, bad)
        assert (lc == lc_o).all() and (w_next.f == f0_o).all() and (w_next.f_coeff == lfo.icrt(f0_o)).all(), j
        rc, lc_v = inst.verify(lfo.Transcript(), acc, cccs_j, proof)
        assert rc == 0 and (lc_v == lc).all(), j
        acc, w_acc = lc, w_next
        acc_o, f_acc = lc_o, lfo.icrt(f0_o)


@pytest.mark.parametrize("name", ["T8", "T8b4"])
@pytest.mark.parametrize("pair", two_sided.SWAP, ids=lambda p: "+".join(p))
def test_sub_provers_with_different_sides_match_fold_step_sections(name, pair):
    """lf_decomposition_prove twice (the left LCCCS with the left witness, the linearized right instance with the right one) and lf_folding_prove(left, right)
    under one transcript give the decomposition and folding sections of the oracle's fold step for that pair"""
    c = two_sided.case(G, name, pair)
    wl, ctx = c.wl, c.ctx
    tr = _tr()
    lbl = lambda t: diag(int.from_bytes(t.encode(), "big") % P)
    tr.absorb_slice(lbl("acc")); tr.absorb_slice(c.acc)
    tr.absorb_slice(lbl("cm_i")); tr.absorb_slice(c.cccs)
    lin, lin_pr = api.LFLinearizationProver.prove(ctx, c.cccs, c.wR, tr)
    lcs_l, dec_l = api.LFDecompositionProver.prove(ctx, c.acc, c.wL, tr)
    lcs_r, dec_r = api.LFDecompositionProver.prove(ctx, lin, c.wR, tr)
    lc_g, w0, fp_g = api.LFFoldingProver.prove(ctx, np.concatenate([lcs_l, lcs_r]), c.wL, c.wR, tr)
    so = two_sided.sections(wl, c.proof)
    assert (lin_pr == so["proof_lin"]).all()
    assert (dec_l == so["proof_dec_left"]).all() and (dec_r == so["proof_dec_right"]).all()
    assert (fp_g == np.concatenate([so["proof_fold_msgs"], so["proof_theta"], so["proof_eta"]])).all()
    assert (lc_g == c.lc).all() and (w0.f == c.f0).all() and (w0.f_coeff == lfo.icrt(c.f0)).all()


@pytest.mark.parametrize("pair", two_sided.SWAP, ids=lambda p: "+".join(p))
def test_fold_sumcheck_on_device_built_fhat_of_two_witnesses(pair):
    """lf_sumcheck_fold_* on T8b4: slots 5.. hold the f-hat tables of the K parts of the left witness, then of the K parts of the right one, built on the device
    in one call; every round message (2 b + 1 evaluations) against the oracle's sumcheck on the numpy tables of the oracle's parts"""
    c = two_sided.case(G, "T8b4", pair)
    wl, ctx, ref = c.wl, c.ctx, c.ref
    m, tau, K2 = wl.m, wl.tau, 2 * wl.K
    parts = c.wL.decompose(ctx) + c.wR.decompose(ctx)
    tables = torch.zeros((5 + K2 * tau, m, wl.RE), dtype=torch.int64, device="cuda")
    head = rand_ring(77, 5 * m, wl).reshape(5, m, wl.RE)
    for idx, sd in ((0, 1), (2, 2), (4, 3)):
        head[idx] = lfo.build_eq(np.stack([embed(ch) for ch in rand_ring(100 + sd, wl.s, wl)[:, :tau]]))
    tables[:5] = torch.from_numpy(np.ascontiguousarray(head).view(np.int64)).cuda()
    api.get_fhat(ctx, parts, device=tables[5:])
    pl, pr = oracle_parts(lfo, wl, ref.L.f, 0), oracle_parts(lfo, wl, ref.R.f, 0)
    assert (pl != pr).any()
    tab_np = np.concatenate([head] + [fhat_np(p, wl) for p in list(pl) + list(pr)])
    assert (tables.cpu().numpy().view(np.uint64) == tab_np).all()
    mu = rand_ring(9, K2, wl)[:, :tau].copy()
    msgs_o, pt_o = ref.shape.inst.sumcheck_fold(lfo.Transcript(), tab_np, np.stack([embed(ch) for ch in mu]))
    sc = api.MLSumcheckFold(ctx, tables, mu)
    npts = 2 * wl.b + 1
    try:
        for rnd in range(wl.s):
            ev = sc.prove_round(None if rnd == 0 else pt_o[rnd - 1][:tau])
            assert ev.shape[0] == npts and (ev == msgs_o[rnd * npts:(rnd + 1) * npts]).all(), f"round {rnd + 1}"
    finally:
        sc.end()
