"""The z_k build on the int8 matrix cores (csrc/lf_zk_i8.hip, k_recompose_crt_i8) through a whole fold step: proof (u_s and eta read every word of z_k
against the pseudo-random q_j = M_j^T eq(r)), folded LCCCS and folded witness (f_coeff, f, w_ccs, all rows) word for word against the CPU oracle, then
again with the butterfly kernel (LF_ZK_VALU), with LF_EVALS_ONE_STREAM, and with both.  (LF_EVALS_ONE_STREAM belonged to the q_j gathers on the auxiliary
stream, measured and rejected -- DESIGN section 12 --: the library does not read it, and those two runs repeat the first two.)

The two sides fold DIFFERENT witnesses (the base witness and step 1 of the chain).  Shapes: T8 (wit_len = 64: two exact 32-element tiles), T10 (256: several
waves and two blocks per class), R61 (wit_len = 61: the last tile has 29 live lanes of 32, and the rows of z_k are 63 words long: 8-byte aligned only),
G5 (L = 5: the launcher declines and the result is unchanged)."""
import numpy as np
import pytest

import lfo
from latticefold_amd import api
from latticefold_amd.workload import CONFIGS, P, chain_w_ccs, make_workload

pytestmark = pytest.mark.gpu

R61 = (8, 61, 4, 1 << 16, 2, 16, 4)     # (s, wit_len, L, B, b, K, kappa): N = 244, n = 63
SHAPES = ["T8", "T10", "R61", "G5"]
SWITCHES = ("LF_ZK_VALU", "LF_EVALS_ONE_STREAM")

_refs = {}


def _reference(name):
    """the workload and the oracle's fold step, computed once per shape and left unchanged"""
    if name not in _refs:
        wl = make_workload(name)
        inst = lfo.Instance(wl)
        A = inst.ajtai_matrix()
        f_acc = inst.witness_from_w_ccs(wl.w_ccs)
        w1 = chain_w_ccs(wl, 1)
        f_1 = inst.witness_from_w_ccs(w1)
        cm = lambda f: np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
        acc, _ = inst.linearize(lfo.Transcript(), cm(f_acc), f_acc)
        cccs = cm(f_1)
        lc, f0, proof = inst.fold_step(lfo.Transcript(), A, acc, f_acc, cccs, f_1)
        f0c = lfo.icrt(f0)
        w0 = lfo.crt(lfo.recompose(f0c, wl.B, wl.L))
        _refs[name] = (wl, A, w1, acc, cccs, {"lc": lc, "proof": proof, "f": f0, "f_coeff": f0c.reshape(-1, 24), "w_ccs": w0.reshape(-1, 24)})
    return _refs[name]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _run(ref, env, monkeypatch):
    wl, A, w1, acc, cccs, _ = ref
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "1")
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


@pytest.mark.parametrize("name", SHAPES)
def test_fold_step_i8_z_matches_the_oracle_under_every_switch(name, monkeypatch):
    monkeypatch.setitem(CONFIGS, "R61", R61)
    ref = _reference(name)
    want = ref[-1]
    for env in ((), SWITCHES[:1], SWITCHES[1:], SWITCHES):
        got = _run(ref, env, monkeypatch)
        for key in ("proof", "lc", "f_coeff", "f", "w_ccs"):
            _same(got[key], want[key], f"{name} {key} vs the oracle ({' '.join(env) or 'default'})")
