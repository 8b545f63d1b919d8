"""Decomposition bases b = 4, 8, 16 on the device (Goldilocks, one GPU): lf_fold_step and the component entry points, bit-exact against the CPU oracle, which is
written for any b (oracle/lfo_protocol.c).  Every test here needs lf_ccs_load to accept b != 2.

Part commitments "at the limits": with a power-of-two B the value whose K digits are ALL +-b/2, (b/2)(b^K - 1)/(b - 1), lies outside a witness handle's bound
B/2, so it cannot reach the kernels through the ABI; the extreme a handle can hold is +-B/2 = +-(b/2) b^(K-1) (b 4 / 16, K 8 / 4), whose top part is all +-b/2
-- that is what the limit tests commit, next to ragged N, both kappa and edge residues in A."""
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import lfo
from latticefold_amd import api
from latticefold_amd.workload import P, RE, diag, make_workload, splitmix_fq
from two_sided import sections as _sections

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_base_digests.json")
UNSUPPORTED = -3


def _wl(name, K=None, kappa=None):
    wl = make_workload(name, 0, kappa=kappa)
    if K is not None:
        wl.K = K
    return wl


class Case:
    def __init__(self, wl, mode=0, matrix=None):
        self.wl = wl
        self.ctx = api.Context(0)
        if mode:
            self.ctx.set_digit_mode(mode)
        self.ctx.load_ccs(wl)
        if matrix is None:
            self.scheme = api.AjtaiCommitmentScheme(self.ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        else:
            self.scheme = api.AjtaiCommitmentScheme(self.ctx, matrix=matrix)

    def close(self):
        self.ctx.close()


def _tr():
    return api.PoseidonTranscript()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def _digests(wl, acc, lc, f0, proof):
    d = {k: _sha(v) for k, v in _sections(wl, proof).items()}
    d.update({"acc": _sha(acc), "lcccs_out": _sha(lc), "f0_ntt": _sha(f0)})
    return d


def _gpu_step(case):
    wit = api.Witness.from_w_ccs(case.ctx, case.wl.w_ccs)
    cccs = np.concatenate([wit.commit(case.scheme), case.wl.x_ccs])
    acc, _ = api.LFLinearizationProver.prove(case.ctx, cccs, wit, _tr())
    lc, w0, proof = api.NIFSProver.prove(case.ctx, acc, wit, cccs, wit, _tr())
    return wit, cccs, acc, lc, w0, proof


def _oracle_step(wl, mode=0):
    lfo.set_digit_mode(mode)
    try:
        inst = lfo.Instance(wl)
        A = inst.ajtai_matrix()
        f = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
        acc, _ = inst.linearize(lfo.Transcript(), cccs, f)
        lc, f0, proof = inst.fold_step(lfo.Transcript(), A, acc, f, cccs, f)
    finally:
        lfo.set_digit_mode(0)
    return inst, A, f, cccs, acc, lc, f0, proof


def _assert_step_equal(wl, got, want):
    wit, cccs, acc, lc, w0, proof = got
    inst, A, f, cccs_o, acc_o, lc_o, f0_o, proof_o = want
    assert (cccs == cccs_o).all() and (acc == acc_o).all()
    so, sg = _sections(wl, proof_o), _sections(wl, proof)
    bad = [k for k in so if not (so[k] == sg[k]).all()]
    assert not bad, f"{wl.name}: proof sections differing from the oracle: {bad}"
    assert (lc == lc_o).all()
    assert (w0.f == f0_o).all()
    assert (w0.f_coeff == lfo.icrt(f0_o)).all()
    assert (w0.w_ccs == lfo.crt(lfo.recompose(lfo.icrt(f0_o), wl.B, wl.L))).all()


@pytest.mark.parametrize("name,K,mode", [("T8b4", None, 0), ("T8b8", None, 0), ("T8b16", None, 0), ("C1b4", None, 0), ("C2b4", None, 0), ("C2b16", None, 0),
                                         ("T8b4", 9, 1), ("T8b16", 5, 1)])
def test_fold_step_bit_exact_vs_oracle(name, K, mode):
    wl = _wl(name, K)
    case = Case(wl, mode)
    try:
        _assert_step_equal(wl, _gpu_step(case), _oracle_step(wl, mode))
    finally:
        case.close()


@pytest.mark.parametrize("name", ["C2b4", "C2b16"])
def test_fold_step_matches_committed_oracle_digests(name):
    want = json.load(open(GOLD))[name]
    wl = _wl(name)
    case = Case(wl)
    try:
        wit, cccs, acc, lc, w0, proof = _gpu_step(case)
        got = _digests(wl, acc, lc, w0.f, proof)
        bad = [k for k in want if k in got and got[k] != want[k]]
        assert not bad, f"{name}: sections differing from the oracle fixture: {bad}"
        assert set(got) <= set(want)
    finally:
        case.close()


@pytest.mark.parametrize("name", ["T8b4", "C1b4"])
def test_components_match_oracle(name):
    wl = _wl(name)
    case = Case(wl)
    try:
        inst, A, f, cccs, acc, lc_o, f0_o, proof_o = _oracle_step(wl)
        wit = api.Witness.from_w_ccs(case.ctx, wl.w_ccs)
        # lf_decomposition_prove: the K LCCCS and the proof (u_s, v_s, x_s, y_s)
        lcs_o, dec_o = inst.decomposition_prove(lfo.Transcript(), A, acc, f)
        lcs_g, dec_g = api.LFDecompositionProver.prove(case.ctx, acc, wit, _tr())
        assert (dec_g == dec_o).all() and (lcs_g == lcs_o).all()
        # lf_sumcheck_fold_*: random tables, driven round by round with the oracle's challenges, 2b + 1 evaluations each
        m, tau, K2 = wl.m, wl.tau, 2 * wl.K
        nt = 5 + K2 * tau
        tables = splitmix_fq(77, 0, nt * m * RE).reshape(nt, m, RE)
        emb = lambda c: np.tile(np.asarray(c, dtype=np.uint64), 8)
        for idx, sd in ((0, 1), (2, 2), (4, 3)):
            pt = splitmix_fq(100 + sd, 0, wl.s * tau).reshape(wl.s, tau)
            tables[idx] = lfo.build_eq(np.stack([emb(c) for c in pt]))
        mu = splitmix_fq(9, 0, K2 * tau).reshape(K2, tau)
        msgs_o, pt_o = inst.sumcheck_fold(lfo.Transcript(), tables, np.stack([emb(c) for c in mu]))
        sc = api.MLSumcheckFold(case.ctx, tables, mu)
        npts = 2 * wl.b + 1
        for rnd in range(wl.s):
            ev = sc.prove_round(None if rnd == 0 else pt_o[rnd - 1][:tau])
            assert ev.shape[0] == npts and (ev == msgs_o[rnd * npts:(rnd + 1) * npts]).all(), f"round {rnd + 1}"
        sc.end()
    finally:
        case.close()


@pytest.mark.parametrize("name", ["T8b4", "C1b4"])
def test_folding_prove_matches_fold_step_sections(name):
    """lf_decomposition_prove twice and lf_folding_prove under one transcript give the decomposition and folding sections of the oracle's fold step"""
    wl = _wl(name)
    case = Case(wl)
    try:
        inst, A, f, cccs, acc, lc_o, f0_o, proof_o = _oracle_step(wl)
        wit = api.Witness.from_w_ccs(case.ctx, wl.w_ccs)
        tr = _tr()
        lbl = lambda t: diag(int.from_bytes(t.encode(), "big") % P)
        tr.absorb_slice(lbl("acc")); tr.absorb_slice(acc)
        tr.absorb_slice(lbl("cm_i")); tr.absorb_slice(cccs)
        lin, _ = api.LFLinearizationProver.prove(case.ctx, cccs, wit, tr)
        # (transcript order of the step: left parts are absorbed after the linearization)
        lcs_l, dec_l = api.LFDecompositionProver.prove(case.ctx, acc, wit, tr)
        lcs_r, dec_r = api.LFDecompositionProver.prove(case.ctx, lin, wit, tr)
        lc_g, w0, fp_g = api.LFFoldingProver.prove(case.ctx, np.concatenate([lcs_l, lcs_r]), wit, wit, tr)
        so = _sections(wl, proof_o)
        assert (dec_l == so["proof_dec_left"]).all() and (dec_r == so["proof_dec_right"]).all()
        assert (fp_g == np.concatenate([so["proof_fold_msgs"], so["proof_theta"], so["proof_eta"]])).all()
        assert (lc_g == lc_o).all() and (w0.f == f0_o).all()
    finally:
        case.close()


def _edge_matrix(kappa, n):
    A = splitmix_fq(0xA11CE, 0, kappa * n * RE).reshape(kappa, n, RE)
    edge = np.array([0, 1, P - 1, (P - 1) // 2, (P + 1) // 2], dtype=np.uint64)
    flat = A.reshape(-1)
    flat[::7] = edge[np.arange(flat[::7].size) % 5]
    return A


@pytest.mark.parametrize("b,K,mode,sign", [(4, None, 0, 1), (4, None, 0, -1), (16, None, 0, 1), (16, None, 0, -1), (4, 9, 1, -1), (16, 5, 1, -1)])
@pytest.mark.parametrize("kappa,shape", [(1, "R61"), (26, "R61"), (26, "T8")])
def test_part_commitments_at_the_limits(b, K, mode, sign, kappa, shape):
    """every coefficient +-B/2: the top part is all +-b/2 (rule 1: -b/2 only); N = 4 * 61 = 244 is ragged (not a multiple of the 8-column tile); kappa 1 and the
    C4 value 26; A with residues 0, 1, p - 1, (p +- 1) / 2 among random ones.  y_s of lf_decomposition_prove against the oracle's (lfo_ajtai_commit of each part)."""
    wl = _wl(f"{shape}b{b}", K, kappa=kappa)
    A = _edge_matrix(kappa, wl.N)
    case = Case(wl, mode, matrix=A)
    try:
        v = wl.B // 2 if sign > 0 else P - wl.B // 2
        f = np.full((wl.N, RE), v, dtype=np.uint64)
        f[1::3] = splitmix_fq(5, 0, f[1::3].size).reshape(f[1::3].shape) % np.uint64(wl.B // 2)   # (ordinary columns in between)
        wit = api.Witness.from_f_coeff(case.ctx, f)
        lfo.set_digit_mode(mode)
        try:
            parts = lfo.decompose(f, wl.b, wl.K, 1).reshape(wl.K, wl.N, RE)
            top = parts[wl.K - 1 if mode == 0 else [k for k in range(wl.K) if (parts[k][0] != 0).any()][-1]][0::3]
            dg = wl.b // 2 if sign > 0 else P - wl.b // 2
            assert (top == dg).all()
            y = [lfo.ajtai_commit(A, kappa, wl.N, lfo.crt(parts[k])) for k in range(wl.K)]
        finally:
            lfo.set_digit_mode(0)
        cm = lfo.ajtai_commit(A, kappa, wl.N, lfo.crt(f))
        acc = np.zeros((case.ctx.lcccs_len, RE), dtype=np.uint64)
        pt = splitmix_fq(3, 0, wl.s * 3).reshape(wl.s, 3)
        acc[:wl.s] = np.tile(pt, (1, 8))
        acc[wl.s + 3:wl.s + 3 + kappa] = cm
        acc[-1] = np.tile(np.array([1, 0, 0], dtype=np.uint64), 8)
        _, dec = api.LFDecompositionProver.prove(case.ctx, acc, wit, _tr())
        y_g = dec[wl.K * (wl.t + wl.tau + wl.l + 1):].reshape(wl.K, kappa, RE)
        for k in range(1, wl.K):
            assert (y_g[k] == y[k]).all(), f"part {k}"
        assert (y_g[0] == y[0]).all()   # the fix-up with powers of b
    finally:
        case.close()


def test_product_checks_on_the_folded_output():
    wl = _wl("C2b4")
    case = Case(wl)
    try:
        wit, cccs, acc, lc, w0, proof = _gpu_step(case)
        ok, lc_v, _ = api.NIFSVerifier.verify(wl, acc, cccs, proof, _tr())
        assert ok and (lc_v == lc).all()
        assert (w0.commit(case.scheme) == lc[wl.s + 3:wl.s + 3 + wl.kappa]).all()       # the folded witness opens the folded commitment
        assert case.ctx.check_lcccs(lc, w0, wl.B // 2) == set()
        fc = w0.f_coeff.copy()
        fc[7, 3] = (int(fc[7, 3]) + 1) % P
        assert case.ctx.check_lcccs(lc, api.Witness.from_f_coeff(case.ctx, fc), wl.B // 2) != set()
    finally:
        case.close()


def _load_rc(ctx, wl):
    try:
        ctx.load_ccs(wl)
    except api.LfError as e:
        return e.code
    return 0


def test_refusals():
    for b in (3, 32):
        wl = _wl("T8b4")
        wl.b = b
        ctx = api.Context(0)
        try:
            assert _load_rc(ctx, wl) == UNSUPPORTED
        finally:
            ctx.close()
    # b = 4, K = 8 under digit rule 1: at the load when the rule is set first, at the step when it changes afterwards
    wl = _wl("T8b4")
    ctx = api.Context(0)
    try:
        ctx.set_digit_mode(1)
        assert _load_rc(ctx, wl) == UNSUPPORTED
    finally:
        ctx.close()
    case = Case(wl)
    try:
        wit = api.Witness.from_w_ccs(case.ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(case.scheme), wl.x_ccs])
        acc, _ = api.LFLinearizationProver.prove(case.ctx, cccs, wit, _tr())
        case.ctx.set_digit_mode(1)
        with pytest.raises(api.LfError) as e:
            api.NIFSProver.prove(case.ctx, acc, wit, cccs, wit, _tr())
        assert e.value.code == UNSUPPORTED
        with pytest.raises(api.LfError) as e:
            api.LFDecompositionProver.prove(case.ctx, acc, wit, _tr())
        assert e.value.code == UNSUPPORTED
    finally:
        case.close()
    # BabyBear and sharded contexts keep refusing b != 2
    wb = make_workload("B6", 0)
    wb.b, wb.K = 4, 8
    ctx = api.Context(0, ring="babybear")
    try:
        assert _load_rc(ctx, wb) == UNSUPPORTED
    finally:
        ctx.close()
    ctx = api.Context(0)
    try:
        ctx.set_sharding_model(0, 2)
        assert _load_rc(ctx, _wl("T8b4")) == UNSUPPORTED
        assert _load_rc(ctx, make_workload("T8", 0)) == 0
    finally:
        ctx.close()


def test_b2_is_untouched_next_to_small_base_contexts():
    """T8 and C2 steps still equal the oracle in a process where b > 2 steps have run on a sibling context; two contexts with different b run concurrently"""
    sib = Case(_wl("T8b16"))
    try:
        _gpu_step(sib)
        for name in ("T8", "C2"):
            wl = _wl(name)
            case = Case(wl)
            try:
                _assert_step_equal(wl, _gpu_step(case), _oracle_step(wl))
            finally:
                case.close()
        _gpu_step(sib)
    finally:
        sib.close()
    cases = [Case(_wl("T8")), Case(_wl("T8b4"))]
    try:
        want = [_oracle_step(c.wl) for c in cases]
        errs = []

        def work(i):
            try:
                for _ in range(3):
                    _assert_step_equal(cases[i].wl, _gpu_step(cases[i]), want[i])
            except BaseException as e:  # noqa: BLE001
                errs.append((i, repr(e)[:300]))

        ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
    finally:
        for c in cases:
            c.close()
