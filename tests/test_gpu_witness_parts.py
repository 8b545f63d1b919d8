"""The decomposed witnesses on the device: lf_witness_decompose / lf_witness_recompose / lf_decomposition_prove_parts / lf_folding_prove_parts
(decompose_witness, nifs/decomposition.rs:162-167; the w_s of LFFoldingProver::prove, nifs/folding.rs:42-130).

The yardstick is the CPU oracle: lfo.decompose(f, b, K, 1) under lfo.set_digit_mode, lfo.recompose + lfo.crt for w_ccs and f; everything is compared word for
word.  tests/test_witness_parts_cpu.py checks what this file takes from the oracle for granted."""
import ctypes as C

import numpy as np
import pytest

from latticefold_amd import api
from latticefold_amd.workload import RE, diag
from witness_parts_cases import CASES, CASE_IDS, edge_f_coeff, oracle_for, oracle_parts, oracle_witness, residues, workload

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, NORM, STATE = -1, -3, -5, -7
u64p = C.POINTER(C.c_uint64)
SENTINEL = 0xDEAD0


class Case:
    def __init__(self, wl, mode=0, scheme=True):
        self.wl = wl
        self.ctx = api.Context(0, ring=wl.ring)
        if mode:
            self.ctx.set_digit_mode(mode)
        self.ctx.load_ccs(wl)
        self.scheme = api.AjtaiCommitmentScheme(self.ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed()) if scheme else None

    def tr(self):
        return api.PoseidonTranscript(ring=self.wl.ring)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def refs():
    """per case, computed once and never written to: the two input witnesses (f_coeff) and their oracle parts"""
    out = {}
    for name, K, mode in CASES:
        wl = workload(name, K)
        lfo = oracle_for(wl)
        fs = [oracle_witness(lfo, wl, mode), edge_f_coeff(wl)]
        ps = [oracle_parts(lfo, wl, f, mode) for f in fs]
        for a in fs + ps:
            a.setflags(write=False)
        out[(name, K, mode)] = (wl, fs, ps)
    return out


def _free(wits):
    for w in wits:
        if w is not None:
            w.free()


@pytest.mark.parametrize("name,K,mode", CASES, ids=CASE_IDS)
def test_parts_equal_the_oracle(refs, name, K, mode):
    wl, fs, ps = refs[(name, K, mode)]
    lfo = oracle_for(wl)
    case = Case(wl, mode)
    try:
        for which, (f, want) in enumerate(zip(fs, ps)):
            wit = api.Witness.from_w_ccs(case.ctx, wl.w_ccs) if which == 0 else api.Witness.from_f_coeff(case.ctx, f)
            assert (wit.f_coeff == f).all()
            parts = wit.decompose(case.ctx)
            assert len(parts) == wl.K
            for k, part in enumerate(parts):
                assert (part.f_coeff == want[k]).all(), f"input {which}, part {k}: f_coeff"
                assert (part.f == lfo.crt(want[k])).all(), f"input {which}, part {k}: f"
                assert (part.w_ccs == lfo.crt(lfo.recompose(want[k], wl.B, wl.L))).all(), f"input {which}, part {k}: w_ccs"
            if which == 1:   # one commitment per configuration: the part that holds the low digits of every edge
                A = lfo.Instance(wl).ajtai_matrix()
                assert (parts[0].commit(case.scheme) == lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(want[0]))).all()
            # the round trip: the parts are the decomposition of their sum, so the sum comes back
            back = api.Witness.recompose(case.ctx, parts)
            assert (back.f_coeff == f).all(), f"input {which}: recompose(decompose(w)) != w"
            _free(parts + [back, wit])
    finally:
        case.close()


def test_sharded_context_cuts_and_joins_the_same(refs):
    """witnesses are replicated and the work is local: rank 1 of 2 gives the parts of an unsharded context"""
    wl, fs, ps = refs[("T8", None, 0)]
    ctx = api.Context(0)
    try:
        ctx.set_sharding_model(1, 2)
        ctx.load_ccs(wl)
        wit = api.Witness.from_f_coeff(ctx, fs[1])
        parts = wit.decompose(ctx)
        assert all((part.f_coeff == ps[1][k]).all() for k, part in enumerate(parts))
        assert (api.Witness.recompose(ctx, parts).f_coeff == fs[1]).all()
    finally:
        ctx.close()


def _linearized(case):
    wl = case.wl
    wit = api.Witness.from_w_ccs(case.ctx, wl.w_ccs)
    cccs = np.concatenate([wit.commit(case.scheme), wl.x_ccs])
    acc, _ = api.LFLinearizationProver.prove(case.ctx, cccs, wit, case.tr())
    return wit, cccs, acc


@pytest.mark.parametrize("name", ["T8", "T8b4", "B6"])
def test_each_decomposed_instance_is_satisfied_by_its_part(name):
    wl = workload(name)
    case = Case(wl)
    try:
        wit, cccs, acc = _linearized(case)
        t1, t2 = case.tr(), case.tr()
        lcs, proof, parts = api.LFDecompositionProver.prove_parts(case.ctx, acc, wit, t1)
        lcs0, proof0 = api.LFDecompositionProver.prove(case.ctx, acc, wit, t2)
        assert (lcs == lcs0).all() and (proof == proof0).all()
        assert (t1.get_challenge() == t2.get_challenge()).all()
        ll = case.ctx.lcccs_len
        inst = lambda k: lcs[k * ll:(k + 1) * ll]
        for k in range(wl.K):
            assert case.ctx.check_lcccs(inst(k), parts[k], wl.b // 2 + 1) == set(), f"part {k}"
        assert case.ctx.check_lcccs(inst(0), parts[1], wl.b // 2 + 1) != set()
        assert case.ctx.check_lcccs(inst(1), parts[0], wl.b // 2 + 1) != set()
    finally:
        case.close()


def _two_decompositions(case, wit, cccs, acc):
    """the transcript of a fold step up to the folding prover: (transcript, the 2K decomposed LCCCS)"""
    tr = case.tr()
    ring = case.wl.ring
    lbl = lambda t: diag(int.from_bytes(t.encode(), "big") % case.wl.P, ring)
    tr.absorb_slice(lbl("acc")); tr.absorb_slice(acc)
    tr.absorb_slice(lbl("cm_i")); tr.absorb_slice(cccs)
    lin, _ = api.LFLinearizationProver.prove(case.ctx, cccs, wit, tr)
    lcs_l, _ = api.LFDecompositionProver.prove(case.ctx, acc, wit, tr)
    lcs_r, _ = api.LFDecompositionProver.prove(case.ctx, lin, wit, tr)
    return tr, np.concatenate([lcs_l, lcs_r])


@pytest.mark.parametrize("name", ["T8", "T8b4", "B6"])
def test_folding_prove_parts_equals_folding_prove(name):
    wl = workload(name)
    case = Case(wl)
    try:
        wit, cccs, acc = _linearized(case)
        ta, lcs = _two_decompositions(case, wit, cccs, acc)
        tb = ta.clone()
        w_s = wit.decompose(case.ctx) + wit.decompose(case.ctx)
        lc_a, w_a, pr_a = api.LFFoldingProver.prove(case.ctx, lcs, wit, wit, ta)
        lc_b, w_b, pr_b = api.LFFoldingProver.prove_parts(case.ctx, lcs, w_s, tb)
        assert (lc_a == lc_b).all() and (pr_a == pr_b).all()
        assert (w_a.f == w_b.f).all() and (w_a.f_coeff == w_b.f_coeff).all()
        assert (ta.get_challenge() == tb.get_challenge()).all()
    finally:
        case.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def _handles(wits):
    return (C.c_void_p * max(len(wits), 1))(*[w.h.value for w in wits])


def _raw_recompose(ctx, wits, count=None):
    """(return code, the output handle) of lf_witness_recompose with the output preset to a sentinel"""
    h = C.c_void_p(SENTINEL)
    rc = api._lib().lf_witness_recompose(ctx.h, _handles(wits), len(wits) if count is None else count, C.byref(h))
    return rc, h.value


def _raw_fold_parts(case, lcs, wits, tr):
    ctx, prm = case.ctx, case.ctx.params
    lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
    pr = np.zeros((prm.s * (2 * prm.b + 1) + 2 * prm.K * (ctx.TAU + prm.t), ctx.RE), dtype=np.uint64)
    h = C.c_void_p(SENTINEL)
    a = np.ascontiguousarray(lcs, dtype=np.uint64)
    rc = api._lib().lf_folding_prove_parts(ctx.h, tr.h, a.ctypes.data_as(u64p), _handles(wits), len(wits), lc.ctypes.data_as(u64p), C.byref(h), pr.ctypes.data_as(u64p))
    return rc, h.value


def _raw_dec_parts(case, acc, wit, tr):
    ctx, prm = case.ctx, case.ctx.params
    lcs = np.zeros((prm.K * ctx.lcccs_len, ctx.RE), dtype=np.uint64)
    pr = np.zeros((prm.K * (prm.t + ctx.TAU + prm.l + 1 + prm.kappa), ctx.RE), dtype=np.uint64)
    hs = (C.c_void_p * prm.K)(*([SENTINEL] * prm.K))
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    rc = api._lib().lf_decomposition_prove_parts(ctx.h, tr.h, a.ctypes.data_as(u64p), wit.h, lcs.ctypes.data_as(u64p), pr.ctypes.data_as(u64p), hs)
    return rc, list(hs)


def _const(case, v):
    """the witness whose every coefficient is v"""
    return api.Witness.from_f_coeff(case.ctx, residues(np.full((case.wl.N, case.wl.RE), v), case.wl.P))


def _fold_step_equals_oracle(case, want):
    wit, cccs, acc = _linearized(case)
    lc, w0, proof = api.NIFSProver.prove(case.ctx, acc, wit, cccs, wit, case.tr())
    acc_o, lc_o, f0_o, proof_o = want
    assert (acc == acc_o).all() and (lc == lc_o).all() and (proof == proof_o).all() and (w0.f == f0_o).all()


@pytest.fixture(scope="module")
def oracle_steps():
    import lfo
    out = {}
    for name in ("T8", "T8b4"):
        wl = workload(name)
        inst = lfo.Instance(wl)
        A = inst.ajtai_matrix()
        f = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
        acc, _ = inst.linearize(lfo.Transcript(), cccs, f)
        lc, f0, proof = inst.fold_step(lfo.Transcript(), A, acc, f, cccs, f)
        out[name] = (acc, lc, f0, proof)
    return out


def _refused_everywhere(case, lcs, tr, left, right, code):
    """one bad left half: lf_witness_recompose and lf_folding_prove_parts refuse it with `code`, return no handle and leave the transcript alone"""
    assert _raw_recompose(case.ctx, left) == (code, None)
    before = tr.clone().get_challenge()
    assert _raw_fold_parts(case, lcs, left + right, tr) == (code, None)
    assert _raw_fold_parts(case, lcs, right + left, tr) == (code, None)      # (the fresh instance's half is looked at as well)
    assert (tr.clone().get_challenge() == before).all()


@pytest.mark.parametrize("name", ["T8", "T8b4"])
def test_refusals(oracle_steps, name):
    wl = workload(name)
    case, other = Case(wl), Case(wl, scheme=False)
    b, K = wl.b, wl.K
    try:
        wit, cccs, acc = _linearized(case)
        tr, lcs = _two_decompositions(case, wit, cccs, acc)
        good = wit.decompose(case.ctx)
        zero = _const(case, 0)
        # wrong count
        assert _raw_recompose(case.ctx, good[:-1]) == (INVALID, None)
        assert _raw_recompose(case.ctx, good + [zero]) == (INVALID, None)
        assert _raw_fold_parts(case, lcs, good + good[:-1], tr) == (INVALID, None)
        # a part of another context
        foreign = api.Witness.from_w_ccs(other.ctx, wl.w_ccs).decompose(other.ctx)
        _refused_everywhere(case, lcs, tr, good[:-1] + [foreign[-1]], good, INVALID)
        with pytest.raises(api.LfError) as e:
            foreign[0].decompose(case.ctx)
        assert e.value.code == INVALID
        # one illegal digit: b/2 + 1 in part 0
        _refused_everywhere(case, lcs, tr, [_const(case, b // 2 + 1)] + [zero] * (K - 1), good, INVALID)
        _refused_everywhere(case, lcs, tr, [zero] * (K - 1) + [_const(case, -(b // 2) - 1)], good, INVALID)
        if b == 4:   # a tie on the wrong side: 2 = (-2) + 1 * 4, legal digits, but the decomposition of 2 is (+2, 0, ..)
            _refused_everywhere(case, lcs, tr, [_const(case, -2), _const(case, 1)] + [zero] * (K - 2), good, INVALID)
            ok = api.Witness.recompose(case.ctx, [_const(case, 2)] + [zero] * (K - 1))
            assert (ok.f_coeff == _const(case, 2).f_coeff).all()
        else:        # b = 2: a digit against the sign of its value, 1 = (-1) + 1 * 2; and all-ones parts, the decomposition of 2^16 - 1 > B/2
            _refused_everywhere(case, lcs, tr, [_const(case, -1), _const(case, 1)] + [zero] * (K - 2), good, INVALID)
            assert (K, wl.B) == (16, 1 << 16)
            _refused_everywhere(case, lcs, tr, [_const(case, 1)] * K, good, NORM)
        # lf_decomposition_prove_parts: a witness of another context; no handle comes back, nothing is absorbed
        before = tr.clone().get_challenge()
        rc, hs = _raw_dec_parts(case, acc, foreign[0], tr)
        assert rc == INVALID and hs == [None] * K and (tr.clone().get_challenge() == before).all()
        if name == "T8b4":   # the digit rule changed after the load: K = 8 digits of base 4 do not cover B/2 under rule 1
            case.ctx.set_digit_mode(1)
            with pytest.raises(api.LfError) as e:
                wit.decompose(case.ctx)
            assert e.value.code == UNSUPPORTED
            assert _raw_recompose(case.ctx, good) == (UNSUPPORTED, None)
            assert _raw_fold_parts(case, lcs, good + good, tr) == (UNSUPPORTED, None)
            rc, hs = _raw_dec_parts(case, acc, wit, tr)
            assert rc == UNSUPPORTED and hs == [None] * K
            assert (tr.clone().get_challenge() == before).all()
            case.ctx.set_digit_mode(0)
        # the good parts still fold, and the context still proves what the oracle proves
        ta = tr.clone()
        lc_a, w_a, pr_a = api.LFFoldingProver.prove(case.ctx, lcs, wit, wit, ta)
        lc_b, w_b, pr_b = api.LFFoldingProver.prove_parts(case.ctx, lcs, good + good, tr)
        assert (lc_a == lc_b).all() and (pr_a == pr_b).all() and (w_a.f == w_b.f).all()
        _fold_step_equals_oracle(case, oracle_steps[name])
    finally:
        case.close()
        other.close()


def test_no_constraint_system():
    wl = workload("T8")
    bare, case = api.Context(0), Case(wl, scheme=False)
    try:
        assert _raw_recompose(bare, []) == (STATE, None)
        h = C.c_void_p(SENTINEL)
        z = np.zeros(RE, dtype=np.uint64)
        tr = api.PoseidonTranscript()
        rc = api._lib().lf_folding_prove_parts(bare.h, tr.h, z.ctypes.data_as(u64p), _handles([]), 0, z.ctypes.data_as(u64p), C.byref(h), z.ctypes.data_as(u64p))
        assert (rc, h.value) == (STATE, None)
        wit = api.Witness.from_w_ccs(case.ctx, wl.w_ccs)   # (no witness can belong to a context without a CCS: a foreign one is refused as foreign)
        assert api._lib().lf_witness_decompose(bare.h, wit.h, (C.c_void_p * 1)()) == INVALID
    finally:
        bare.close()
        case.close()
