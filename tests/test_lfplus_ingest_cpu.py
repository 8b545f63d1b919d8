"""Instance ingestion of the LatticeFold+ slice (lfplus_witness_from_z / lfplus_commit_resident: ComR1CS::new on the device), the parts that need no GPU: the
two entry points exist in every layer (header, shared library, generated Rust binding, ctypes mirror), and the host restatement of
Vec<R>::gadget_decompose agrees with the oracle's digit rule on the edge values -- the convention the device kernel (lfp_ingest.hip) must reproduce."""
import os
import re

import numpy as np
import pytest

import lfp
from latticefold_amd import plus

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
P, D = plus.P, 16
BASES = (2, 3, 7, 8, 16, 3108, 3109, 1 << 20, 1 << 31)
KS = (1, 2, 4, 16)


def edge_values(b, k):
    """0, 1, p - 1, (p +- 1) / 2, +- b/2, +- (b/2 + 1), +- (b^k - 1)/2, +- b^k/2, +- (b^k/2 + 1) (those below p/2) as canonical words"""
    vals = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
    for m in (b // 2, b // 2 + 1, (b ** k - 1) // 2, b ** k // 2, b ** k // 2 + 1):
        if m < P // 2:
            vals += [m, (P - m) % P]
    return np.array(sorted(set(vals)), dtype=np.uint64)


def edge_z(b, k, m, seed=0):
    """m ring elements whose coefficients run through edge_values(b, k) (every value at every coefficient position when m allows)"""
    ev = edge_values(b, k)
    idx = (np.arange(m * D, dtype=np.int64).reshape(m, D) + np.arange(m, dtype=np.int64)[:, None] * 5 + seed) % ev.size
    return ev[idx]


def test_entry_points_exist_in_every_layer():
    names = ("lfplus_witness_from_z", "lfplus_commit_resident")
    hdr = open(os.path.join(ROOT, "include", "lfplus.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    lib = plus._lib()
    for n in names:
        assert re.search(r"\bint %s\(lfplus_ctx \*ctx" % n, hdr), f"{n} is not declared in include/lfplus.h"
        assert n in plus.exported_symbols()
        assert hasattr(lib, n), f"liblfhip.so does not export {n}"
        assert re.search(r"pub fn %s\(" % n, rs), f"{n} is missing from the generated Rust binding"
        assert getattr(lib, n).argtypes is not None, f"{n} has no argtypes in plus.py"
    assert len(lib.lfplus_witness_from_z.argtypes) == 6 and len(lib.lfplus_commit_resident.argtypes) == 2
    for meth in ("witness_from_z", "commit_resident"):
        assert callable(getattr(plus.PlusContext, meth))
    assert callable(plus.ComR1CS.new_resident) and callable(plus.ComR1CS.fetch_f) and callable(plus.PlusProver.ingest)


@pytest.mark.parametrize("b", BASES)
def test_host_gadget_decompose_equals_the_oracle_on_edge_values(b):
    rng = np.random.default_rng(b % 1000)
    for k in KS:
        z = np.concatenate([edge_z(b, k, 24), rng.integers(0, P, size=(8, D), dtype=np.uint64)])
        got, want = plus.gadget_decompose(z, b, k), lfp.gadget_decompose(z, b, k)
        assert got.shape == want.shape == (z.shape[0] * k, D)
        assert (got == want).all(), (b, k)
