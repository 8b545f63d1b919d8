"""q_j = M_j^T eq(r) gathered straight into the packed int8 operand of the u_s / eta inner products (csrc/lf_dot_i8.hip, k_q_pack_i8) through a whole fold
step over the C ABI: proof (u_s of both sides and eta are those inner products), folded LCCCS and folded witness (f_coeff, f, w_ccs) word for word against the
CPU oracle -- once by default and once under LF_Q_TWO_PASS (the gathers into 64-bit words and k_dot_pack_y behind them).  LF_DOT_MIN=64 sends these small
shapes to the int8 form.  The two sides fold DIFFERENT witnesses (the base witness and step 1 of the chain, or an all-zero one).

Shapes: T8 (n = 66: one full block of 64 columns and a block of two), T10 (n = 258: several blocks, a partial last one), T10 multi4 (several non-zeros per
column, ring-valued entries, columns without a non-zero), R61 (n = 63 < 64: the shape test declines, the words are produced as before), T10 deg3 (t = 4: two
groups of two in the dot call, the two-pass form is kept), T8 with an all-zero incoming witness (its z_k rows are zero beyond the head)."""
import numpy as np
import pytest

import lfo
from latticefold_amd import api
from latticefold_amd.workload import CONFIGS, P, chain_w_ccs, make_workload

pytestmark = pytest.mark.gpu

R61 = (8, 61, 4, 1 << 16, 2, 16, 4)     # (s, wit_len, L, B, b, K, kappa): N = 244, n = 63
CASES = [("T8", "r1cs", False), ("T10", "r1cs", False), ("T10", "multi4", False), ("R61", "r1cs", False), ("T10", "deg3", False), ("T8", "r1cs", True)]
N_COLS = {"T8": 66, "T10": 258, "R61": 63}

_refs = {}


def _reference(name, ccs, zero):
    """the workload and the oracle's fold step, computed once per case and left unchanged"""
    key = (name, ccs, zero)
    if key not in _refs:
        wl = make_workload(name, ccs=ccs)
        assert wl.n == N_COLS[name]
        inst = lfo.Instance(wl)
        A = inst.ajtai_matrix()
        f_acc = inst.witness_from_w_ccs(wl.w_ccs)
        w1 = np.zeros_like(wl.w_ccs) if zero else chain_w_ccs(wl, 1)
        f_1 = inst.witness_from_w_ccs(w1)
        cm = lambda f: np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
        acc, _ = inst.linearize(lfo.Transcript(), cm(f_acc), f_acc)
        cccs = cm(f_1)
        lc, f0, proof = inst.fold_step(lfo.Transcript(), A, acc, f_acc, cccs, f_1)
        f0c = lfo.icrt(f0)
        w0 = lfo.crt(lfo.recompose(f0c, wl.B, wl.L))
        _refs[key] = (wl, A, w1, acc, cccs, {"lc": lc, "proof": proof, "f": f0, "f_coeff": f0c.reshape(-1, 24), "w_ccs": w0.reshape(-1, 24)})
    return _refs[key]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _run(ref, two_pass, monkeypatch):
    wl, A, w1, acc, cccs, _ = ref
    monkeypatch.setenv("LF_DOT_MIN", "64")
    monkeypatch.delenv("LF_DOT_VALU", raising=False)
    if two_pass:
        monkeypatch.setenv("LF_Q_TWO_PASS", "1")
    else:
        monkeypatch.delenv("LF_Q_TWO_PASS", raising=False)
    ctx = api.Context(0)
    try:
        ctx.load_ccs(wl)
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)   # noqa: F841 (installs the commitment matrix of the step)
        wa, wi = api.Witness.from_w_ccs(ctx, wl.w_ccs), api.Witness.from_w_ccs(ctx, w1)
        lc, w0, proof = api.NIFSProver.prove(ctx, acc, wa, cccs, wi, api.PoseidonTranscript())
        # canonical residues: the NTT words of the folded witness may be any representative
        return {"lc": lc, "proof": proof, "f": np.array(w0.f) % np.uint64(P), "f_coeff": np.array(w0.f_coeff), "w_ccs": np.array(w0.w_ccs) % np.uint64(P)}
    finally:
        ctx.close()


@pytest.mark.parametrize("name,ccs,zero", CASES)
def test_fold_step_with_q_gathered_into_digits_matches_the_oracle(name, ccs, zero, monkeypatch):
    monkeypatch.setitem(CONFIGS, "R61", R61)
    ref = _reference(name, ccs, zero)
    want = ref[-1]
    for two_pass in (False, True):
        got = _run(ref, two_pass, monkeypatch)
        for key in ("proof", "lc", "f_coeff", "f", "w_ccs"):
            _same(got[key], want[key], f"{name} {ccs}{' zero witness' if zero else ''} {key} vs the oracle ({'LF_Q_TWO_PASS' if two_pass else 'default'})")
