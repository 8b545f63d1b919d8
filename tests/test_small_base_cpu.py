"""Decomposition bases b = 4, 8, 16 on the host side (no GPU): the oracle's prover and verifier, lf_verify_host and the wire format are written for any b and
are the yardstick of the device path (tests/test_gpu_small_base.py); plus the coverage arithmetic of lf_ccs_load's envelope check."""
import numpy as np
import pytest

import lfo
from latticefold_amd import api
from latticefold_amd.workload import P, make_workload


def _step(name):
    wl = make_workload(name, 0)
    inst = lfo.Instance(wl)
    A = wl.ajtai_matrix()
    f = inst.witness_from_w_ccs(wl.w_ccs)
    cccs = np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
    acc, _ = inst.linearize(lfo.Transcript(), cccs, f)
    lc, f0, proof = inst.fold_step(lfo.Transcript(), A, acc, f, cccs, f)
    return wl, inst, acc, cccs, lc, proof


@pytest.mark.parametrize("name", ["T8b4", "T8b8", "T8b16"])
def test_oracle_step_verifies_on_both_verifiers(name):
    wl, inst, acc, cccs, lc, proof = _step(name)
    assert proof.shape[0] == inst.proof_len
    rc, lc_v = inst.verify(lfo.Transcript(), acc, cccs, proof)
    assert rc == 0 and (lc_v == lc).all()
    back = api.proof_from_bytes(wl, api.proof_to_bytes(wl, proof))
    assert (back == proof).all()
    ok, lc_h, _ = api.NIFSVerifier.verify(wl, acc, cccs, back, api.PoseidonTranscript())
    assert ok and (lc_h == lc).all()
    # one word of the folding-sumcheck section (its first message, 2b + 1 evaluations per round)
    lin = wl.s * (wl.d + 2) + wl.tau + wl.t
    dec = wl.K * (wl.t + wl.tau + wl.l + 1 + wl.kappa)
    bad = proof.copy()
    pos = lin + 2 * dec + wl.b
    bad[pos, 5] = (int(bad[pos, 5]) + 1) % P
    rc, _ = inst.verify(lfo.Transcript(), acc, cccs, bad)
    assert rc != 0
    ok = api.NIFSVerifier.verify(wl, acc, cccs, bad, api.PoseidonTranscript())[0]
    assert not ok


def digits_cover(b, K, B, mode):
    """K balanced base-b digits reach +-(b/2)(b^K - 1)/(b - 1) under rule 0 and only +(b/2 - 1)(b^K - 1)/(b - 1) on the positive side under rule 1; a witness
    handle holds |coefficient| <= B/2 (lf_sb.h sb_digits_cover)."""
    geo = (b**K - 1) // (b - 1)
    if b == 2:
        return geo >= B // 2
    return ((b // 2) if mode == 0 else (b // 2 - 1)) * geo >= B // 2


def test_coverage_arithmetic():
    assert (4**8 - 1) // 3 * 2 == 43690 and (4**8 - 1) // 3 * 1 == 21845
    assert digits_cover(4, 8, 1 << 16, 0)
    assert not digits_cover(4, 8, 1 << 16, 1)
    assert digits_cover(4, 9, 1 << 16, 1)
    assert digits_cover(8, 5, 1 << 15, 0) and digits_cover(16, 4, 1 << 16, 0)
    assert not digits_cover(16, 4, 1 << 16, 1) and digits_cover(16, 5, 1 << 16, 1)
    assert digits_cover(2, 16, 1 << 16, 0) and digits_cover(2, 16, 1 << 16, 1) and not digits_cover(2, 15, 1 << 16, 0)
    # the oracle's digits agree: the extreme values have an exact K-digit form exactly when covered
    for b, K, B, mode in [(4, 8, 1 << 16, 0), (4, 8, 1 << 16, 1), (4, 9, 1 << 16, 1), (16, 4, 1 << 16, 1), (16, 5, 1 << 16, 1)]:
        lfo.set_digit_mode(mode)
        try:
            x = np.zeros((1, 24), dtype=np.uint64)
            x[0, 0] = B // 2
            x[0, 1] = P - B // 2
            d = lfo.decompose(x, b, K, 0)
            exact = (lfo.recompose(d, b, K) == x).all()
        finally:
            lfo.set_digit_mode(0)
        assert exact == digits_cover(b, K, B, mode), (b, K, B, mode)
