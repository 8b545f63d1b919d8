"""The generic sumcheck without a GPU: the eight entry points through every layer (header, library, Python, generated Rust module, INTEGRATION.md, safe crate),
lf_mlsumcheck_verify against the Python reference verifier of tests/mlsumcheck_ref.py on both rings, the refusals that need no device, and the reference
checking itself (extract_sum is the brute-force sum over the hypercube, g on the final values is the verifier's expected evaluation)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import mlsumcheck_ref as ref
from latticefold_amd import api
from latticefold_amd.workload import RINGS

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMBOLS = ["lf_mlsumcheck_begin", "lf_mlsumcheck_begin_device", "lf_mlsumcheck_round", "lf_mlsumcheck_final", "lf_mlsumcheck_end", "lf_mlsumcheck_prove",
           "lf_mlsumcheck_prove_device", "lf_mlsumcheck_verify"]
INVALID, HIP, UNSUPPORTED, REJECT = -1, -2, -3, -8
BOTH = pytest.mark.parametrize("ring", ["goldilocks", "babybear"])


def _gen():
    spec = importlib.util.spec_from_file_location("gen_rust_bindings", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_the_eight_symbols_through_every_layer():
    main = open(os.path.join(ROOT, "include", "lfhip.h")).read()
    assert main.index('extern "C" {') < main.index('#include "lfhip_sumcheck.h"') < main.rindex("#ifdef __cplusplus"), "included inside the extern C block"
    assert "lf_mlsumcheck" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S), "no prototype of it is written into lfhip.h itself"
    assert api.exported_symbols("lfhip_sumcheck.h") == sorted(SYMBOLS)
    assert not set(SYMBOLS) & set(api.exported_symbols()) and not set(SYMBOLS) & set(api.exported_symbols("lfhip_parts.h"))
    lib = api._lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)
    gen = _gen()
    text, fns = gen.generate_sumcheck()
    assert sorted(fns) == sorted(SYMBOLS)
    assert open(gen.SUMCHECK_OUT).read() == text, "run tools/gen_rust_bindings.py --write"
    doc = open(gen.DOC).read()
    block = doc[doc.index(gen.SUMCHECK_BEGIN) + len(gen.SUMCHECK_BEGIN):doc.index(gen.SUMCHECK_END)]
    assert block.strip() == ("```rust\n" + text + "```").strip(), "INTEGRATION.md: the sumcheck block is stale"
    assert "pub struct lf_vpoly" in text and "pub mod sumcheck;" in open(gen.OUT).read()
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read()
    assert "sys::sumcheck::lf_mlsumcheck_prove(" in safe and "sys::sumcheck::lf_mlsumcheck_verify(" in safe
    assert re.search(r"pub fn prove_as_subprotocol\(", safe) and re.search(r"pub fn verify_as_subprotocol\(", safe) and "pub struct HipMLSumcheck" in safe


# ---- lf_mlsumcheck_verify against the Python reference ----------------------------------------------------------------------------------------------------
def _small(ring, kind):
    """(tables, terms, degree, nvars) of the verifier cases"""
    RE = RINGS[ring][1]
    if kind == "deg3":
        return ref.SHAPES["b"](3, ring) + (3,)
    c = ref.rand_ring(0x51, (2, RE), ring)
    if kind == "deg1":
        return ref.rand_ring(0x52, (2, 4, RE), ring), [(c[0], [0]), (c[1], [1])], 1, 2
    if kind == "deg8":   # (claimed degree 8, the polynomial's own degree 2: every message is a polynomial of lower degree than claimed)
        return ref.rand_ring(0x53, (3, 4, RE), ring), [(c[0], [0, 1]), (c[1], [2])], 8, 2
    raise KeyError(kind)


def _both_verifiers(ring, nvars, degree, claim, msgs):
    O = ref.oracle(ring)
    tr_o, tr = O.Transcript(), api.PoseidonTranscript(ring=ring)
    want = ref.verify(tr_o, nvars, degree, claim, msgs, ring)
    got = api.MLSumcheck.verify(tr, nvars, degree, claim, msgs, ring=ring)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) if want[0] else got[2] == want[2]
    assert np.array_equal(tr.get_challenge(), tr_o.challenge()), "the transcript has advanced as the reference's has"
    return got


@BOTH
@pytest.mark.parametrize("kind", ["deg3", "deg1", "deg8"])
def test_verify_against_the_reference(ring, kind):
    tables, terms, degree, nvars = _small(ring, kind)
    msgs, point, final = ref.prove(ref.oracle(ring).Transcript(), tables, terms, degree, ring)
    claim = api.MLSumcheck.extract_sum(msgs)
    # the reference checks itself
    assert np.array_equal(claim, ref.hypercube_sum(tables, terms, ring))
    ok, pt, exp = _both_verifiers(ring, nvars, degree, claim, msgs)
    assert ok and np.array_equal(pt, point) and np.array_equal(exp, ref.g_at(final, terms, ring))
    # one word of round 2 changed: rejected there
    bad = msgs.copy()
    bad[1, 1, 5] ^= np.uint64(1)
    ok, _, where = _both_verifiers(ring, nvars, degree, claim, bad)
    assert not ok and where == 1
    tr = api.PoseidonTranscript(ring=ring)
    rc = api._lib().lf_mlsumcheck_verify(api.RING_IDS[ring], tr.h, nvars, degree, api._a64(claim)[1], api._a64(bad)[1],
                                         np.zeros((nvars, RINGS[ring][2]), dtype=np.uint64).ctypes.data_as(api.u64p),
                                         np.zeros(RINGS[ring][1], dtype=np.uint64).ctypes.data_as(api.u64p))
    assert rc == REJECT
    # an evaluation beyond the first two changed in round 1: the sum check of round 1 still holds, round 2 fails
    if degree >= 2:
        bad = msgs.copy()
        bad[0, 2, 0] ^= np.uint64(1)
        ok, _, where = _both_verifiers(ring, nvars, degree, claim, bad)
        assert not ok and where == 1
    # a wrong claimed sum: rejected at round 0
    wrong = claim.copy()
    wrong[3] ^= np.uint64(1)
    ok, _, where = _both_verifiers(ring, nvars, degree, wrong, msgs)
    assert not ok and where == 0


@BOTH
def test_verify_refusals(ring):
    p, RE, TAU = RINGS[ring]
    L = api._lib()
    tables, terms, degree, nvars = _small(ring, "deg1")
    msgs, _, _ = ref.prove(ref.oracle(ring).Transcript(), tables, terms, degree, ring)
    claim = api.MLSumcheck.extract_sum(msgs)
    po, eo = np.zeros((nvars, TAU), dtype=np.uint64), np.zeros(RE, dtype=np.uint64)
    outs = (po.ctypes.data_as(api.u64p), eo.ctypes.data_as(api.u64p))
    tr = api.PoseidonTranscript(ring=ring)
    fresh = api.PoseidonTranscript(ring=ring).get_challenge()
    pc, pm = api._a64(claim)[1], api._a64(msgs)[1]
    rid = api.RING_IDS[ring]
    assert L.lf_mlsumcheck_verify(rid, None, nvars, degree, pc, pm, *outs) == INVALID
    assert L.lf_mlsumcheck_verify(rid, tr.h, nvars, degree, None, pm, *outs) == INVALID
    assert L.lf_mlsumcheck_verify(rid, tr.h, nvars, degree, pc, None, *outs) == INVALID
    assert L.lf_mlsumcheck_verify(rid, tr.h, nvars, degree, pc, pm, None, outs[1]) == INVALID
    assert L.lf_mlsumcheck_verify(7, tr.h, nvars, degree, pc, pm, *outs) == INVALID
    assert L.lf_mlsumcheck_verify(1 - rid, tr.h, nvars, degree, pc, pm, *outs) == INVALID          # a transcript of the other ring
    big = msgs.copy(); big[1, 0, 2] = p
    assert L.lf_mlsumcheck_verify(rid, tr.h, nvars, degree, pc, api._a64(big)[1], *outs) == INVALID
    for nv, dg in ((0, 1), (31, 1), (nvars, 0), (nvars, 9)):
        assert L.lf_mlsumcheck_verify(rid, tr.h, nv, dg, pc, pm, *outs) == UNSUPPORTED
    assert np.array_equal(tr.get_challenge(), fresh), "a refused call leaves the transcript alone"


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_before_any_device_is_touched():
    L = api._lib()
    ring = "goldilocks"
    tables, terms, degree, nvars = _small(ring, "deg1")
    good = api.VPoly(terms, degree).desc(ring, nvars, 2)
    bad_index = api.VPoly([(terms[0][0], [0]), (terms[1][0], [2])], degree).desc(ring, nvars, 2)
    pt = api._a64(tables)[1]
    assert L.lf_mlsumcheck_begin(None, C.byref(good), pt) == INVALID                         # a NULL context
    assert L.lf_mlsumcheck_begin(None, None, pt) == INVALID                                  # a NULL descriptor
    assert L.lf_mlsumcheck_begin(None, C.byref(bad_index), pt) == INVALID                    # an index >= T
    assert L.lf_mlsumcheck_begin_device(None, C.byref(good), None) == INVALID
    tr = api.PoseidonTranscript(ring=ring)
    o = np.zeros(4 * 24 * 4, dtype=np.uint64).ctypes.data_as(api.u64p)
    assert L.lf_mlsumcheck_prove(None, tr.h, C.byref(good), pt, o, o, o) == INVALID
    assert L.lf_mlsumcheck_prove_device(None, tr.h, C.byref(good), None, o, o, o) == INVALID
    assert L.lf_mlsumcheck_round(None, None, o) == INVALID and L.lf_mlsumcheck_final(None, o, o) == INVALID and L.lf_mlsumcheck_end(None) == INVALID
    import torch
    if not torch.cuda.is_available():                                                        # no CPU fallback: the wrapper's prove ends in LF_ERR_HIP
        with pytest.raises(api.LfError) as e:
            ctx = api.Context(0, ring=ring)
            api.MLSumcheck.prove(ctx, tr, tables, api.VPoly(terms, degree))
        assert e.value.code == HIP


def test_vpoly_descriptor():
    ring = "babybear"
    p, RE, tau = RINGS[ring]
    g = ref.rand_ring(9, (RE,), ring)
    vp = api.VPoly([(g, [0, 1, 1]), (-1, [2]), (5, [0])])
    assert vp.degree == 3
    d = vp.desc(ring, 4, 3)
    assert (d.nvars, d.ntables, d.nterms, d.degree) == (4, 3, 3, 3)
    assert [d.term_off[i] for i in range(4)] == [0, 3, 4, 5] and [d.term_idx[i] for i in range(5)] == [0, 1, 1, 2, 0]
    coef = np.ctypeslib.as_array(d.coef, shape=(3, RE))
    assert np.array_equal(coef[0], g) and (coef[1, ::tau] == p - 1).all() and coef[1].sum() == 8 * (p - 1) and (coef[2, ::tau] == 5).all()


# ---- the reference checks itself -------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape,nvars", [("a", 3), ("b", 2), ("e", 3), ("f-mix", 3)])
def test_the_reference_checks_itself(ring, shape, nvars):
    tables, terms, degree = ref.SHAPES[shape](nvars, ring)
    O = ref.oracle(ring)
    msgs, point, final = ref.prove(O.Transcript(), tables, terms, degree, ring)
    claim = api.MLSumcheck.extract_sum(msgs)
    assert np.array_equal(claim, ref.hypercube_sum(tables, terms, ring)), "extract_sum is the brute-force sum of g over the hypercube"
    ok, pt, expected = ref.verify(O.Transcript(), nvars, degree, claim, msgs, ring)
    assert ok and np.array_equal(pt, point)
    assert np.array_equal(ref.g_at(final, terms, ring), expected), "g on the final values is the verifier's expected evaluation"
    # the final values are the tables' multilinear extensions at the point, variable 1 in bit 0: sum_x eq(point, x) T[x]
    one = ref.ext_embed_int(1, ring)
    w = one[None]
    for r in point:                                                              # eq weights, lowest variable first
        e = ref.embed(r, ring)
        w = np.concatenate([ref.ring_mul_ntt(w, ref.rsub(one, e, ring), ring), ref.ring_mul_ntt(w, e, ring)], axis=0)
    # (concatenation puts the newest variable in the HIGHEST bit of the index: variable i of the point is bit i of x)
    for j in range(tables.shape[0]):
        assert np.array_equal(ref.rsum(ref.ring_mul_ntt(w, tables[j], ring), ring), final[j])
