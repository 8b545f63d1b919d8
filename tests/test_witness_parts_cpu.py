"""The oracle-side facts tests/test_gpu_witness_parts.py leans on, and the Python surface of the decomposed witnesses (no GPU).

For every (B, b, K) of the GPU cases and every digit rule under which K digits cover B/2: the parts lfo.decompose(f, b, K, 1) gives recompose to f exactly (centred
lifts) and lie in the rule's range -- so "equal to the oracle's parts" is "the decomposition".  The two constructions lf_witness_recompose must refuse really are
what the GPU test says they are."""
import importlib.util
import os
import re

import numpy as np
import pytest

from latticefold_amd import api
from witness_parts_cases import CASES, CASE_IDS, centred, digits_cover, edge_f_coeff, oracle_for, oracle_parts, oracle_witness, residues, workload


@pytest.mark.parametrize("name,K,mode", CASES, ids=CASE_IDS)
def test_oracle_parts_recompose_exactly_and_stay_in_range(name, K, mode):
    wl = workload(name, K)
    lfo = oracle_for(wl)
    assert digits_cover(wl.b, wl.K, wl.B, mode)
    for rule in (0, 1):
        if not digits_cover(wl.b, wl.K, wl.B, rule):
            continue   # (the load refuses this pair: T8b8 / T8b16 / R61b4 at their own K under rule 1)
        for f in (edge_f_coeff(wl), oracle_witness(lfo, wl, rule)):
            fc = centred(f, wl.P)
            assert abs(fc).max() <= wl.B // 2
            parts = centred(oracle_parts(lfo, wl, f, rule), wl.P)
            assert (sum(parts[k] * wl.b**k for k in range(wl.K)) == fc).all()
            half = wl.b // 2
            assert parts.min() >= -half and parts.max() <= (half - 1 if rule == 1 and wl.b > 2 else half)
            if wl.b == 2:   # sign and bits of the magnitude: no digit against the sign of its value
                assert (parts * np.sign(fc)[None] >= 0).all()


def test_edge_inputs_hold_the_edges():
    for name, K, _ in CASES:
        wl = workload(name, K)
        fc = centred(edge_f_coeff(wl), wl.P)
        want = {0, 1, -1, 2, -2, wl.b // 2, -(wl.b // 2), wl.B // 2 - 1, -(wl.B // 2 - 1), -(wl.B // 2)} | ({wl.B // 2} if wl.B < 1 << 32 else set())
        assert want <= set(fc.reshape(-1).tolist())
        assert (fc.max() < 1 << 31) and fc.min() >= -(1 << 31)


def test_the_refused_constructions():
    import lfo
    # b = 4, rule 0: the value 2 is (+2, 0, ..); (-2, +1, 0, ..) has legal digits and the same sum
    wl = workload("T8b4")
    two = residues(np.full((wl.N, wl.RE), 2), wl.P)
    parts = centred(oracle_parts(lfo, wl, two, 0), wl.P)
    assert (parts[0] == 2).all() and (parts[1:] == 0).all()
    assert -2 + 1 * wl.b == 2 and -(wl.b // 2) <= -2 and 1 <= wl.b // 2
    # b = 2, K = 16: all-ones parts are the decomposition of 2^16 - 1, which is over B/2
    wl = workload("T8")
    assert (wl.b, wl.K, wl.B) == (2, 16, 1 << 16)
    ones = residues(np.full((wl.N, wl.RE), 2**16 - 1), wl.P)
    assert (centred(oracle_parts(lfo, wl, ones, 0), wl.P) == 1).all()
    assert 2**16 - 1 > wl.B // 2
    # the digit b/2 + 1 is outside both rules' ranges and inside a witness handle's bound (so lf_witness_from_f_coeff can build it)
    for name in ("T8", "T8b4"):
        wl = workload(name)
        assert wl.b // 2 < wl.b // 2 + 1 <= wl.B // 2


NEW_SYMBOLS = ("lf_witness_decompose", "lf_witness_recompose", "lf_decomposition_prove_parts", "lf_folding_prove_parts")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_header_binding_and_wrapper_agree():
    """the four entry points are declared in include/lfhip_parts.h, which lfhip.h includes inside its extern "C" block; module `parts` of the -sys crate and its
    block in INTEGRATION.md are what the generator makes of that header; the safe crate calls each of them through `sys::parts::`"""
    main = open(os.path.join(ROOT, "include", "lfhip.h")).read()
    assert main.index('#include "lfhip_parts.h"') < main.rindex("#ifdef __cplusplus")
    assert not set(NEW_SYMBOLS) & set(api.exported_symbols())
    spec = importlib.util.spec_from_file_location("gen_rust_bindings", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text, fns = gen.generate_parts()
    assert tuple(fns) == NEW_SYMBOLS
    assert open(gen.PARTS_OUT).read() == text, "run tools/gen_rust_bindings.py --write"
    doc = open(gen.DOC).read()
    block = doc[doc.index(gen.PARTS_BEGIN) + len(gen.PARTS_BEGIN):doc.index(gen.PARTS_END)]
    assert block.strip() == ("```rust\n" + text + "```").strip(), "run tools/gen_rust_bindings.py --write"
    assert "pub mod parts;" in open(gen.OUT).read()
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read()
    assert set(re.findall(r"sys::parts::(lf_[a-z0-9_]+)\(", safe)) == set(NEW_SYMBOLS)
    for name in ("decompose", "recompose", "prove_resident_parts"):
        assert re.search(r"pub fn " + name + r"\(", safe), name
    assert "decompose_to_vec(P::B_SMALL" not in safe     # the host closures of the two trait impls are gone


def test_python_surface_without_gpu():
    for owner, meth in ((api.Witness, "decompose"), (api.Witness, "recompose"), (api.LFDecompositionProver, "prove_parts"), (api.LFFoldingProver, "prove_parts")):
        assert callable(getattr(owner, meth))
    assert set(api.exported_symbols("lfhip_parts.h")) == set(NEW_SYMBOLS)
    assert all(hasattr(api._lib(), s) for s in NEW_SYMBOLS)
    import torch
    if torch.cuda.is_available():
        return
    tr = api.PoseidonTranscript()
    z = np.zeros((4, 24), dtype=np.uint64)
    calls = (lambda c: api.Witness(c, None).decompose(c), lambda c: api.Witness.recompose(c, []),
             lambda c: api.LFDecompositionProver.prove_parts(c, z, None, tr), lambda c: api.LFFoldingProver.prove_parts(c, z, [], tr))
    for call in calls:
        with pytest.raises(api.LfError) as e:
            call(api.Context(0))
        assert e.value.code == -2   # LF_ERR_HIP: there is no CPU path
