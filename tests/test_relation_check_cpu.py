"""Relation checks without a GPU: lf_ccs_check / lf_cccs_check / lf_lcccs_check (CCS::check_relation arith.rs:76-110, R_CCCS, R_LCCCS arith.rs:193-206) are
declared by include/lfhip.h and exported by liblfhip.so; the Python wrappers refuse to run without a GPU (LF_ERR_HIP, no host fallback); and this file's own host
restatement of the CCS residual -- the one tests/test_gpu_relation_check.py compares the device against -- is right on the synthetic workloads."""
import os
import re

import numpy as np
import pytest

from latticefold_amd import api
from latticefold_amd.workload import RINGS, make_workload, ring_mul_ntt

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMS = ("lf_ccs_check", "lf_cccs_check", "lf_lcccs_check")


def spmv_host(wl, j, z):
    """M_j z on the host: the CSR rows of matrix j, slot-wise products (ring_mul_ntt); rows past the matrix are zero"""
    p, d, _tau = RINGS[wl.ring]
    rp, ci, va = (np.asarray(a) for a in (wl.rowptr[j], wl.col[j], wl.val[j]))
    prod = ring_mul_ntt(va.reshape(-1, d), z[ci.astype(np.int64)], wl.ring)      # [nnz][d]
    row = np.repeat(np.arange(wl.m), np.diff(rp.astype(np.int64)))
    out = np.zeros((wl.m, d), dtype=object)
    np.add.at(out, row, prod.astype(object))
    return (out % p).astype(np.uint64)


def residual_host(wl, z):
    """sum_i c_i (.) prod_{j in S_i} M_j z, row by row ([m][d] canonical words)"""
    p, d, _tau = RINGS[wl.ring]
    mz = [spmv_host(wl, j, z) for j in range(wl.t)]
    res = np.zeros((wl.m, d), dtype=object)
    for i in range(wl.q):
        term = np.tile(np.asarray(wl.c[i], dtype=np.uint64), (wl.m, 1))
        for k in range(int(wl.S_off[i]), int(wl.S_off[i + 1])):
            term = ring_mul_ntt(term, mz[int(wl.S_idx[k])], wl.ring)
        res += term.astype(object)
    return (res % p).astype(np.uint64)


def bad_rows(res):
    return np.nonzero(res.any(axis=1))[0]


def referencing_rows(wl, col):
    rows = set()
    for j in range(wl.t):
        rp, ci = np.asarray(wl.rowptr[j]).astype(np.int64), np.asarray(wl.col[j])
        rows |= set(np.repeat(np.arange(wl.m), np.diff(rp))[ci == col].tolist())
    return rows


def test_header_declares_and_library_exports_the_three_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfhip.h")).read(), flags=re.S)
    lib = api._lib()
    for s in SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert s in api.exported_symbols(), s
        assert hasattr(lib, s), s
    for name, bit in (("CM", 1), ("CCS", 2), ("U", 4), ("V", 8), ("NORM", 16)):
        assert re.search(r"\bLF_REL_" + name + r"\s*=\s*" + str(bit) + r"\b", hdr), name
    assert api.REL_BITS == {"cm": 1, "ccs": 2, "u": 4, "v": 8, "norm": 16}
    assert issubclass(api.NotSatisfied, api.LfError)


def test_wrappers_need_a_gpu():
    """without a GPU every path to the checks ends in LF_ERR_HIP (no context can be made; there is no host fallback); with one, a context without a
    constraint system refuses them (LF_ERR_STATE)"""
    import torch
    wl = make_workload("T8")
    if torch.cuda.is_available():
        ctx = api.Context(0)
        try:
            with pytest.raises(api.LfError) as e:
                ctx.check_relation(wl.z())
            assert e.value.code == -7 and not isinstance(e.value, api.NotSatisfied)
        finally:
            ctx.close()
        return
    calls = (lambda c: c.check_relation(wl.z()), lambda c: c.check_cccs(np.zeros((wl.kappa + wl.l, 24), np.uint64), None),
             lambda c: c.check_lcccs(np.zeros((40, 24), np.uint64), None))
    for call in calls:
        with pytest.raises(api.LfError) as e:
            call(api.Context(0))
        assert e.value.code == -2   # LF_ERR_HIP


@pytest.mark.parametrize("name", ["T10", "B8"])
@pytest.mark.parametrize("ccs", ["r1cs", "multi4", "multi16", "deg3"])
def test_host_residual_is_zero_on_the_workloads(name, ccs):
    wl = make_workload(name, ccs=ccs)
    res = residual_host(wl, wl.z())
    assert res.shape == (wl.m, wl.RE) and not res.any()


@pytest.mark.parametrize("name", ["T10", "B8"])
@pytest.mark.parametrize("ccs", ["r1cs", "deg3"])
def test_one_tampered_element_shows_exactly_at_its_rows(name, ccs):
    """one changed w_ccs element: the residual is non-zero exactly at the rows whose matrices reference its column (r1cs, deg3: every such row depends on
    it non-trivially; the multi* systems stay satisfied in a referencing row whose own z_i is unchanged)"""
    wl = make_workload(name, ccs=ccs)
    z = wl.z().copy()
    col = wl.l + 1 + 7
    z[col, 0] = (int(z[col, 0]) + 1) % wl.P
    refs = referencing_rows(wl, col)
    got = set(bad_rows(residual_host(wl, z)).tolist())
    assert refs and got == refs, (sorted(got), sorted(refs))
