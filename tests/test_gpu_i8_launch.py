"""The launch path of the int8 matrix-core commit kernels (lf_i8_launch.h): the 160 KB LDS opt-in is made per (kernel, device), so a process with contexts
on two devices computes the same words on both; and the commit switches are read per call (Tunables), so flipping LF_I8_COUPLE_W between calls of one
process takes effect in either order.  Outputs are compared word for word with the oracle, as tests/test_gpu_ajtai_i8.py does."""
import os

import numpy as np
import pytest
import torch

from latticefold_amd import api
from latticefold_amd.workload import make_workload

pytestmark = pytest.mark.gpu


def _run(name, device):
    """Witness.commit (k_ajtai_i8g) + linearization + LFDecompositionProver.prove (the digit-plane commit kernels) on one device"""
    wl = make_workload(name)
    tr = lambda: api.PoseidonTranscript(ring=wl.ring)
    ctx = api.Context(device, ring=wl.ring)
    try:
        ctx.load_ccs(wl)
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=wl.ajtai_matrix())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr())
        dec = api.LFDecompositionProver.prove(ctx, acc, wit, tr())
    finally:
        ctx.close()
    return cccs, dec


def _want(name, cccs):
    """the oracle's decomposition of the instance whose CCCS (commitment || x_ccs) the GPU produced"""
    wl = make_workload(name)
    if wl.ring == "goldilocks":
        import lfo as O
    else:
        import lfo_bb as O
    inst = O.Instance(wl)
    f_coeff = inst.witness_from_w_ccs(wl.w_ccs)
    acc_o, _ = inst.linearize(O.Transcript(), cccs, f_coeff)
    return inst.decomposition_prove(O.Transcript(), wl.ajtai_matrix(), acc_o, f_coeff)


def _matches(dec, want):
    return (dec[1] == want[1]).all() and (dec[0] == want[0]).all()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("name", ["T8", "E99", "B14"])
def test_second_device_computes_the_same_words(name):
    """one workload per large-LDS kernel family: the generic k_ajtai_i8 (T8), k_ajtai_i8s (E99: 13 row tiles), k_ajtai_i8x (B14: 72-ring, 4 row tiles);
    Witness.commit reaches k_ajtai_i8g on all of them.  Device 0 first, then device 1, in one process."""
    cccs0, dec0 = _run(name, 0)
    cccs1, dec1 = _run(name, 1)
    assert (cccs1 == cccs0).all()
    assert (dec1[0] == dec0[0]).all() and (dec1[1] == dec0[1]).all()
    want = _want(name, cccs0)
    assert _matches(dec0, want) and _matches(dec1, want)


def test_couple_switch_is_read_per_call():
    """T10 with LF_I8_COUPLE_W = 0, then unset, then 0 again, in one process: every run equals the oracle, whichever value the process saw first.  The coupling
    has no observable but time: that the value reaches the launcher at every call is Tunables::read and the launcher's argument, not this test."""
    saved = os.environ.pop("LF_I8_COUPLE_W", None)
    try:
        runs = []
        for value in ("0", None, "0"):
            if value is None:
                os.environ.pop("LF_I8_COUPLE_W", None)
            else:
                os.environ["LF_I8_COUPLE_W"] = value
            runs.append(_run("T10", 0))
        want = _want("T10", runs[0][0])
        for cccs, dec in runs:
            assert (cccs == runs[0][0]).all()
            assert _matches(dec, want)
    finally:
        os.environ.pop("LF_I8_COUPLE_W", None)
        if saved is not None:
            os.environ["LF_I8_COUPLE_W"] = saved
