"""The wide CCS envelope (t <= 8 matrices, degree d <= 7) on the host side (no GPU): the workload kinds "deg4" .. "deg7" and "mix8", the oracle's prover and
verifier on them, the product's host-only lf_verify_host and the wire format, and the committed oracle-only fixture.  The oracle is generic in t, q and d and is
the yardstick of the device path (tests/test_gpu_wide_ccs.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import lfo
from latticefold_amd import api
from latticefold_amd.workload import CONFIGS, P, make_workload, mix8_gamma
from test_relation_check_cpu import residual_host

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_ccs_digests.json")
KINDS = ["deg4", "deg5", "deg6", "deg7", "mix8"]
SHAPE = {"deg4": (5, 2, 4), "deg5": (6, 2, 5), "deg6": (7, 2, 6), "deg7": (8, 2, 7), "mix8": (8, 3, 5)}   # t, q, d


def residual(wl):
    """sum_i c_i prod_{j in S_i} (M_j z), row by row (the host restatement of tests/test_relation_check_cpu.py)"""
    return residual_host(wl, wl.z())


@pytest.mark.parametrize("name", ["T8", "G5"])
@pytest.mark.parametrize("ccs", KINDS)
def test_workload_kinds_are_satisfied(name, ccs):
    wl = make_workload(name, 0, ccs=ccs)
    assert (wl.t, wl.q, wl.d) == SHAPE[ccs]
    assert len(wl.rowptr) == len(wl.col) == len(wl.val) == wl.t and wl.c.shape == (wl.q, wl.RE)
    assert list(wl.S_idx) == list(range(wl.t)) and int(wl.S_off[-1]) == wl.t
    assert max(int(wl.S_off[i + 1] - wl.S_off[i]) for i in range(wl.q)) == wl.d
    assert not residual(wl).any()
    # one witness element changed: the residual is non-zero exactly in that element's row
    bad = make_workload(name, 0, ccs=ccs)
    bad.w_ccs = bad.w_ccs.copy()
    bad.w_ccs[3, 4] = (int(bad.w_ccs[3, 4]) + 1) % P
    rows = np.nonzero(residual(bad).any(axis=1))[0]
    assert list(rows) == [wl.l + 1 + 3]


def test_mix8_gamma_slots():
    g = mix8_gamma().reshape(8, 3)
    assert len({tuple(int(x) for x in s) for s in g}) == 8
    assert not any(tuple(int(x) for x in s) in ((1, 0, 0), (P - 1, 0, 0)) for s in g)
    wl = make_workload("T8", 0, ccs="mix8")
    assert (wl.c[1] == mix8_gamma()).all() and (wl.c[0].reshape(8, 3) == [1, 0, 0]).all() and (wl.c[2].reshape(8, 3) == [P - 1, 0, 0]).all()


def _workload_digest(wl):
    h = hashlib.sha256()
    for a in [wl.S_off, wl.S_idx, wl.c, wl.w_ccs, wl.x_ccs] + list(wl.rowptr) + list(wl.col) + list(wl.val):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# sha256 over S_off, S_idx, c, w_ccs, x_ccs and every matrix's rowptr / col / val at T8, seed 0, recorded on the commit before the wide kinds were added
EXISTING = {"r1cs": ((3, 2, 2), "8732706884fef71c8747593d38d30c66e64259fa4e9408e4d43814994aeb231a"), "deg3": ((4, 2, 3), "f74921be26bae67f911c6a63d9c3a40bf48795385467613261073edcbb0a4012"), "multi": ((3, 2, 2), "f467d37222686276b292f5704859a6911f80a439f724d510cfa3b324b52a26a5")}


@pytest.mark.parametrize("ccs", sorted(EXISTING))
def test_existing_kinds_are_byte_identical(ccs):
    shape, digest = EXISTING[ccs]
    wl = make_workload("T8", 0, ccs=ccs)
    assert (wl.t, wl.q, wl.d) == shape
    assert _workload_digest(wl) == digest


def _step(name, ccs):
    wl = make_workload(name, 0, ccs=ccs)
    inst = lfo.Instance(wl)
    A = wl.ajtai_matrix()
    f = inst.witness_from_w_ccs(wl.w_ccs)
    cccs = np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
    acc, _ = inst.linearize(lfo.Transcript(), cccs, f)
    lc, f0, proof = inst.fold_step(lfo.Transcript(), A, acc, f, cccs, f)
    return wl, inst, acc, cccs, lc, proof


@pytest.mark.parametrize("ccs", ["deg5", "deg7", "mix8"])
def test_oracle_step_verifies_on_both_verifiers_and_round_trips(ccs):
    wl, inst, acc, cccs, lc, proof = _step("T8", ccs)
    assert proof.shape[0] == inst.proof_len
    rc, lc_v = inst.verify(lfo.Transcript(), acc, cccs, proof)
    assert rc == 0 and (lc_v == lc).all()
    ok, lc_h, stage = api.NIFSVerifier.verify(wl, acc, cccs, proof, api.PoseidonTranscript())
    assert ok and stage == 0 and (lc_h == lc).all()
    back = api.proof_from_bytes(wl, api.proof_to_bytes(wl, proof))
    assert back.shape == proof.shape and (back == proof).all()
    # one word of a linearization message (d + 2 evaluations per round) is caught by both verifiers
    bad = proof.copy()
    bad[wl.d + 1, 5] = (int(bad[wl.d + 1, 5]) + 1) % P
    assert inst.verify(lfo.Transcript(), acc, cccs, bad)[0] != 0
    assert not api.NIFSVerifier.verify(wl, acc, cccs, bad, api.PoseidonTranscript())[0]


def test_committed_fixture_is_consistent():
    gold = json.load(open(GOLD))
    assert set(gold) == {"C2/deg5", "C2/deg7", "C2/mix8"}
    keys = {"acc", "lcccs_out", "f0_ntt", "proof_lin", "proof_dec_left", "proof_dec_right", "proof_fold_msgs", "proof_theta", "proof_eta", "proof"}
    for name, rec in gold.items():
        cfg, ccs = name.split("/")
        wl = make_workload("T8", 0, ccs=ccs)          # (the shape of the kind does not depend on the size)
        assert (rec["t"], rec["q"], rec["d"]) == (wl.t, wl.q, wl.d) == SHAPE[ccs]
        assert keys <= set(rec) and all(len(rec[k]) == 64 for k in keys)
        assert (rec["s"], rec["b"], rec["K"], rec["B"], rec["kappa"]) == (CONFIGS[cfg][0], CONFIGS[cfg][4], CONFIGS[cfg][5], CONFIGS[cfg][3], CONFIGS[cfg][6])
