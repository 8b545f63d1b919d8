"""The LatticeFold+ generic sumcheck without a GPU: the eight entry points in header, library and Python mirror; the Python reference of
tests/lfplus_mlsumcheck_ref.py pinned to the oracle's lfp.r1cs_linearize; lfplus_mlsumcheck_verify (host only) against that reference; the answers of the
device entry points when there is no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfp
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMBOLS = ["lfplus_mlsumcheck_begin", "lfplus_mlsumcheck_begin_device", "lfplus_mlsumcheck_round", "lfplus_mlsumcheck_final", "lfplus_mlsumcheck_end",
           "lfplus_mlsumcheck_prove", "lfplus_mlsumcheck_prove_device", "lfplus_mlsumcheck_verify"]
P, D = plus.P, plus.D
u64p = plus.u64p


def test_the_eight_symbols_through_every_layer():
    names = plus.exported_symbols()
    lib = plus._lib()
    for s in SYMBOLS:
        assert s in names, f"include/lfplus.h does not declare {s}"
        assert hasattr(lib, s), f"liblfhip.so does not export {s}"
    sys_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    assert all(f"pub fn {s}(" in sys_rs for s in SYMBOLS) and "pub struct lfplus_vpoly" in sys_rs
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "plus.rs")).read()
    assert "sys::lfplus_mlsumcheck_prove(" in safe and "sys::lfplus_mlsumcheck_verify(" in safe
    assert re.search(r"pub fn prove_as_subprotocol\(", safe) and re.search(r"pub fn verify_as_subprotocol\(", safe)
    assert all(hasattr(plus, n) for n in ("VPoly", "MLSumcheck", "mlsumcheck_prove", "mlsumcheck_verify"))


def test_vpoly_descriptor():
    g = ref.rand_ring(9, (D,))
    vp = plus.VPoly([(g, [0, 1, 1]), (-1, [2]), (5, [0])])
    assert vp.degree == 3
    d = vp.desc(4, 3)
    assert (d.nvars, d.ntables, d.nterms, d.degree) == (4, 3, 3, 3)
    assert [d.term_off[i] for i in range(4)] == [0, 3, 4, 5] and [d.term_idx[i] for i in range(5)] == [0, 1, 1, 2, 0]
    coef = np.ctypeslib.as_array(d.coef, shape=(3, D))
    assert np.array_equal(coef[0], g) and coef[1, 0] == P - 1 and not coef[1, 1:].any() and coef[2, 0] == 5 and not coef[2, 1:].any()


@pytest.mark.parametrize("nvars", [3, 4])
def test_the_reference_reproduces_the_oracle_linearization(nvars):
    """the schedule of ref.prove on the tables (eq(r, .), M_A f, M_B f, M_C f) with the terms +[0, 1, 2] - [0, 3] at degree 3 gives the words of the oracle's
    ComR1CS::linearize: the messages, the point and va / vb / vc"""
    n = 1 << nvars
    f = ref.rand_ring(0x71 + nvars, (n, D))
    r1cs = [ref.rand_csr(0x72 + 3 * nvars + q, n, 1) for q in range(3)]
    tr_o = lfp.Transcript()
    tr_o.absorb(ref.rand_ring(0x73, (2, D)))
    mine = tr_o.clone()
    want = lfp.r1cs_linearize(tr_o, nvars, f, r1cs)
    r = [mine.challenge() for _ in range(nvars)]                  # as ComR1CS::linearize draws it
    tables = ref.r1cs_tables(r, f, r1cs)
    verifier = mine.clone()
    msgs, point, final = ref.prove(mine, tables, ref.terms_as_rings(ref.R1CS_TERMS), 3)
    assert np.array_equal(msgs, want["msgs"]) and np.array_equal(point, want["r"]) and np.array_equal(final[1:], want["evals"][1:])
    # and the reference checks itself: extract_sum is the brute-force sum, g on the final values is the verifier's expected evaluation
    claim = ref.extract_sum(msgs)
    assert np.array_equal(claim, ref.hypercube_sum(tables, ref.terms_as_rings(ref.R1CS_TERMS)))
    ok, pt, expected = ref.verify(verifier, nvars, 3, claim, msgs)
    assert ok and np.array_equal(pt, point) and np.array_equal(expected, ref.g_at(final, ref.terms_as_rings(ref.R1CS_TERMS)))


def _verify_raw(tr, nvars, degree, claim, msgs):
    point, exp, rnd = np.zeros(nvars, dtype=np.uint64), np.zeros(D, dtype=np.uint64), C.c_int(-7)
    claim, msgs = np.ascontiguousarray(claim, dtype=np.uint64), np.ascontiguousarray(msgs, dtype=np.uint64)
    rc = plus._lib().lfplus_mlsumcheck_verify(tr.h, nvars, degree, claim.ctypes.data_as(u64p), msgs.ctypes.data_as(u64p), point.ctypes.data_as(u64p),
                                              exp.ctypes.data_as(u64p), C.byref(rnd))
    return rc, point, exp, rnd.value


@pytest.mark.parametrize("shape,nvars", [("b", 1), ("a", 2), ("e", 3), ("d", 4), ("f-mix", 3)])
def test_verify_accepts_reference_proofs(shape, nvars):
    tables, terms, degree, msgs, point, final = ref.case(shape, nvars)
    claim = ref.extract_sum(msgs)
    assert np.array_equal(claim, ref.hypercube_sum(tables, terms))
    tr, tr_o = plus.PoseidonTranscript(), lfp.Transcript()
    ok_o, pt_o, exp_o = ref.verify(tr_o, nvars, degree, claim, msgs)
    rc, pt, exp, rnd = _verify_raw(tr, nvars, degree, claim, msgs)
    assert ok_o and rc == 0 and rnd == -1
    assert np.array_equal(pt, point) and np.array_equal(pt, pt_o)
    assert np.array_equal(exp, ref.g_at(final, terms)) and np.array_equal(exp, exp_o)
    assert tr.get_challenge() == tr_o.challenge(), "the transcript has advanced as the oracle's has"
    ok, pt2, exp2 = plus.mlsumcheck_verify(plus.PoseidonTranscript(), nvars, degree, claim, msgs)
    assert ok and np.array_equal(pt2, point) and np.array_equal(exp2, exp)


@pytest.mark.parametrize("nvars", [1, 2, 3, 4])
def test_verify_rejects_a_changed_word(nvars):
    tables, terms, degree, msgs, point, final = ref.case("b", nvars)
    claim = ref.extract_sum(msgs)
    for j in sorted({0, nvars - 1}):
        bad = msgs.copy()
        bad[j, 1, 5] ^= np.uint64(1)
        where = j
        tr, tr_o = plus.PoseidonTranscript(), lfp.Transcript()
        ok_o, _, rnd_o = ref.verify(tr_o, nvars, degree, claim, bad)
        rc, _, exp, rnd = _verify_raw(tr, nvars, degree, claim, bad)
        assert not ok_o and rnd_o == where
        assert rc == plus.E_REJECT and rnd == where and not exp.any()
        assert tr.get_challenge() == tr_o.challenge(), "the transcript has advanced over all rounds"
        ok, _, w = plus.mlsumcheck_verify(plus.PoseidonTranscript(), nvars, degree, claim, bad)
        assert not ok and w == where
    # an evaluation beyond the first two changed in round 1: round 1 still holds, round 2 fails
    if nvars >= 2:
        bad = msgs.copy()
        bad[0, 2, 0] ^= np.uint64(1)
        assert _verify_raw(plus.PoseidonTranscript(), nvars, degree, claim, bad)[::3] == (plus.E_REJECT, 1)
    wrong = claim.copy()
    wrong[3] ^= np.uint64(1)
    assert _verify_raw(plus.PoseidonTranscript(), nvars, degree, wrong, msgs)[::3] == (plus.E_REJECT, 0)


def test_verify_refusals():
    L = plus._lib()
    tables, terms, degree, msgs, point, final = ref.case("b", 2)
    nvars = 2
    claim = ref.extract_sum(msgs)
    po, eo, rnd = np.zeros(nvars, dtype=np.uint64), np.zeros(D, dtype=np.uint64), C.c_int()
    outs = (po.ctypes.data_as(u64p), eo.ctypes.data_as(u64p), C.byref(rnd))
    tr = plus.PoseidonTranscript()
    fresh = plus.PoseidonTranscript().get_challenge()
    m = np.ascontiguousarray(msgs)
    pc, pm = claim.ctypes.data_as(u64p), m.ctypes.data_as(u64p)
    A = plus.E_ARG
    assert L.lfplus_mlsumcheck_verify(None, nvars, degree, pc, pm, *outs) == A
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, None, pm, *outs) == A
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, pc, None, *outs) == A
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, pc, pm, None, outs[1], outs[2]) == A
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, pc, pm, outs[0], None, outs[2]) == A
    big = m.copy(); big[1, 0, 2] = P
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, pc, big.ctypes.data_as(u64p), *outs) == A
    bigc = claim.copy(); bigc[15] = 2**64 - 1
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, bigc.ctypes.data_as(u64p), pm, *outs) == A
    for nv, dg in ((0, degree), (29, degree), (nvars, 0), (nvars, 9)):
        assert L.lfplus_mlsumcheck_verify(tr.h, nv, dg, pc, pm, *outs) == A
    assert tr.get_challenge() == fresh, "a refused call leaves the transcript alone"
    assert L.lfplus_mlsumcheck_verify(tr.h, nvars, degree, pc, pm, outs[0], outs[1], None) in (0, plus.E_REJECT)      # (round may be NULL)
    for nv, dg in ((0, 3), (29, 3), (2, 0), (2, 9)):
        with pytest.raises(plus.LfPlusError) as e:
            plus.mlsumcheck_verify(plus.PoseidonTranscript(), nv, dg, claim, msgs)
        assert e.value.code == A


def test_device_entry_points_without_a_context():
    """a caller without a device holds no context (lfplus_ctx_create said LFPLUS_E_NO_DEVICE): begin and prove answer the same; with a device a NULL context is
    a NULL argument"""
    import torch
    L = plus._lib()
    tables, terms, degree, msgs, point, final = ref.case("b", 2)
    d = plus.VPoly(terms, degree).desc(2, tables.shape[0])
    t = np.ascontiguousarray(tables)
    tr = plus.PoseidonTranscript()
    fresh = plus.PoseidonTranscript().get_challenge()
    o = np.zeros(2 * 4 * D, dtype=np.uint64).ctypes.data_as(u64p)
    want = plus.E_ARG if torch.cuda.is_available() else plus.E_NO_DEVICE
    assert L.lfplus_mlsumcheck_begin(None, C.byref(d), t.ctypes.data_as(u64p)) == want
    assert L.lfplus_mlsumcheck_begin_device(None, C.byref(d), None) == want
    assert L.lfplus_mlsumcheck_prove(None, tr.h, C.byref(d), t.ctypes.data_as(u64p), o, o, o) == want
    assert L.lfplus_mlsumcheck_prove_device(None, tr.h, C.byref(d), None, o, o, o) == want
    assert L.lfplus_mlsumcheck_round(None, None, o) == want and L.lfplus_mlsumcheck_final(None, o, o) == want
    assert L.lfplus_mlsumcheck_end(None) == plus.E_ARG
    assert tr.get_challenge() == fresh
    if not torch.cuda.is_available():                        # no CPU fallback: the wrapper ends where the context is created
        with pytest.raises(plus.LfPlusError) as e:
            plus.mlsumcheck_prove(plus.PlusContext(0), tr, tables, plus.VPoly(terms, degree))
        assert e.value.code == plus.E_NO_DEVICE
