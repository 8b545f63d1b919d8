"""The fold-round kernels on the three-column lazy sums (A3P, LH3, lf_field.cuh): one fold step through every path of modes 6, 7 and 1, bit-exact against the CPU
oracle.  The paths are forced onto oracle-sized workloads with the switches the parity tests use; E22 (N not a multiple of 4) takes the scalar plane loads and
never mode 7.  `pytest -m gpu`."""
import numpy as np
import pytest

import lfo
from fold_paths import A3P_BASE as BASE, A3P_PATHS as PATHS     # the switch sets: rounds 1..3 as GEMMs, then modes 6 / 7 / 1, split and plain
from latticefold_amd import api
from latticefold_amd.workload import make_workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """per workload: the witness on the device, the linearized accumulator and the oracle's fold step, computed once (as test_gpu_parity.run_both does)"""
    memo = {}

    def get(name):
        if name not in memo:
            wl = make_workload(name, 2)
            inst = lfo.Instance(wl)
            ctx.load_ccs(wl)
            A = wl.ajtai_matrix()
            scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
            f_coeff = inst.witness_from_w_ccs(wl.w_ccs)
            wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
            cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
            acc_g, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
            acc_o, _ = inst.linearize(lfo.Transcript(), cccs, f_coeff)
            assert (acc_g == acc_o).all()
            memo[name] = (wl, wit, cccs, acc_g, inst.fold_step(lfo.Transcript(), A, acc_o, f_coeff, cccs, f_coeff))
        return memo[name]
    return get


@pytest.mark.parametrize("name", ["T10", "G5", "E22"])
def test_fold_step_through_the_three_column_paths(ctx, cases, name, monkeypatch):
    wl, wit, cccs, acc_g, (lc_o, f0_o, proof_o) = cases(name)
    m = 1 << wl.s
    for k, v in BASE.items():
        monkeypatch.setenv(k, v)
    # the default thresholds as well; k_lincomb_z (fold prepare, left on its LH5 form) runs in every one of these steps
    for label, (extra, r5, split) in [("default", ({}, False, False))] + list(PATHS.items()):
        for k, v in extra.items():
            monkeypatch.setenv(k, v)
        lc, w, proof = api.NIFSProver.prove(ctx, acc_g, wit, cccs, wit, api.PoseidonTranscript())
        for k in extra:
            monkeypatch.delenv(k)
        assert (proof == proof_o).all() and (lc == lc_o).all() and (w.f == f0_o).all(), (name, label)
        # the intended paths ran: rounds 1..3 as GEMMs wherever 64 pairs remain, and the split mask of the table rounds
        assert ctx.fold_paths() == sum(1 << (r - 1) for r in range(1, 4) if (m >> r) >= 64), (name, label, ctx.fold_paths())
        want_split = 0
        if split and wl.s >= 4:
            want_split |= 0b01000                                   # round 4: mode 6
            if r5 and wl.s >= 5 and wl.N % 4 == 0:
                want_split |= 0b10000                               # round 5: mode 7
        assert ctx.fold_split_rounds() == want_split, (name, label, bin(ctx.fold_split_rounds()))
