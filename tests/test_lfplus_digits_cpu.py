"""Gadget maps on arrays (lfplus_balanced_decompose, lfplus_balanced_recompose, lfplus_linf_norm, their _device forms and lfplus_set_matrices_gadget) without a
GPU: the seven entry points in header, library, Python mirror and the two Rust crates; the answer to a NULL context; and the Python-integer reference of
tests/test_gpu_lfplus_digits.py (tests/lfplus_digits_ref.py) against the definitions the repository already has, on the corner grid."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfp
import lfplus_digits_ref as dref
from latticefold_amd import plus

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PAIRS = [("lfplus_balanced_decompose", "lfplus_balanced_decompose_device"), ("lfplus_balanced_recompose", "lfplus_balanced_recompose_device"),
         ("lfplus_linf_norm", "lfplus_linf_norm_device")]
SYMBOLS = [s for pair in PAIRS for s in pair] + ["lfplus_set_matrices_gadget"]
P, D = plus.P, plus.D
u64p = plus.u64p
SENT = 0x5A5A5A5A5A5A5A5A


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfplus.h")).read(), flags=re.S)


def _params(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, f"include/lfplus.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_seven_symbols_through_every_layer():
    hdr = _header()
    names = plus.exported_symbols()
    lib = plus._lib()
    nm = os.popen("nm -D --defined-only '%s'" % os.path.join(ROOT, "latticefold_amd", "liblfhip.so")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "plus.rs")).read()
    assert len(SYMBOLS) == 7
    for s in SYMBOLS:
        params = _params(hdr, s)
        assert s in names, f"plus.exported_symbols() does not list {s}"
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), f"nm -D of liblfhip.so does not show {s}"
        f = getattr(lib, s)
        assert f.argtypes is not None and len(f.argtypes) == len(params), f"{s} has no ctypes prototype of {len(params)} parameters"
        assert sys_rs.count(f"pub fn {s}(") == 1, f"{s} is not bound exactly once in latticefold-hip-sys"
        assert f"pub fn {s}(" in integ, f"INTEGRATION.md does not list {s}"
        assert f"sys::{s}(" in safe, f"the safe crate does not call {s}"
        assert re.search(r"pub (unsafe )?fn %s[(<]" % s[len("lfplus_"):], safe), f"the safe crate has no wrapper named after {s}"
    for host, device in PAIRS:                                                  # device and host form: one parameter list
        assert _params(hdr, host) == _params(hdr, device)
    assert all(hasattr(plus.PlusContext, n) for n in ("balanced_decompose", "balanced_recompose", "linf_norm", "set_matrices_gadget"))
    assert "LFPLUS_DIGITS_GADGET 0" in hdr and "LFPLUS_DIGITS_PLANES 1" in hdr and (plus.DIGITS_GADGET, plus.DIGITS_PLANES) == (0, 1)


def test_the_section_sits_between_the_tables_and_the_ccs_instances():
    hdr = open(os.path.join(ROOT, "include", "lfplus.h")).read()
    assert hdr.index("MLE tables on arrays:") < hdr.index("gadget maps on arrays:") < hdr.index("committed CCS instances:")
    assert hdr.index("int lfplus_spmv_t_device(") < hdr.index("int lfplus_balanced_decompose(") < hdr.index("int lfplus_set_matrices_gadget(") < hdr.index("} lfplus_ccs;")
    assert not any(s.endswith("_dev") for s in SYMBOLS)
    section = hdr[hdr.index("gadget maps on arrays:"):hdr.index("committed CCS instances:")]
    assert "Not built:" in section and all(w in section for w in ("sharded contexts", "int8 output form", "dense\n * monomials", "prover constructor"))


def test_a_null_context_is_refused_before_any_device_is_touched():
    lib = plus._lib()
    a, out = (np.full((4, D), SENT, dtype=np.uint64) for _ in range(2))
    am = C.c_uint64(SENT)
    pa, po = a.ctypes.data_as(u64p), out.ctypes.data_as(u64p)
    va, vo = C.c_void_p(a.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.lfplus_balanced_decompose(None, pa, 2, 2, 2, 0, po) == plus.E_ARG
    assert lib.lfplus_balanced_decompose_device(None, va, 2, 2, 2, 0, vo) == plus.E_ARG
    assert lib.lfplus_balanced_recompose(None, pa, 2, 2, 2, 1, po) == plus.E_ARG
    assert lib.lfplus_balanced_recompose_device(None, va, 2, 2, 2, 1, vo) == plus.E_ARG
    assert lib.lfplus_linf_norm(None, pa, 4, C.byref(am)) == plus.E_ARG
    assert lib.lfplus_linf_norm_device(None, va, 4, C.byref(am)) == plus.E_ARG
    rp, col, val = plus.identity_csr(4)
    keep, prp, pcol, pval = plus._csr_args([(rp, col, val)])
    before = [x.copy() for x in keep[0]]
    assert lib.lfplus_set_matrices_gadget(None, 4, 4, 2, 2, 8, 1, prp, pcol, pval) == plus.E_ARG
    assert all((x == SENT).all() for x in (a, out)) and am.value == SENT, "the buffers are untouched"
    assert all(np.array_equal(x, y) for x, y in zip(keep[0], before))


def test_truncating_division_written_out():
    for a in (0, 1, -1, 7, -7, 8, -8, 2**63 - 1, -(2**63 - 1)):
        for b in (2, 3, 7, 2**62):
            q, r = dref.tdivmod(a, b)
            assert q * b + r == a and abs(r) < b and (r == 0 or (r > 0) == (a > 0)) and abs(q) == abs(a) // b


@pytest.mark.parametrize("b", dref.BASES)
def test_the_reference_is_the_digit_rule_the_repository_already_has(b):
    """on the corner grid: the oracle's lfp_balanced_digits (tests/lfp.py) and plus.gadget_decompose cut the digits the reference cuts, in gadget order; the
    planes are their transposition"""
    for k in dref.DIGITS:
        x = np.array(dref.corner_values(b, k) + [0] * (-len(dref.corner_values(b, k)) % D), dtype=np.uint64).reshape(-1, D)
        want = dref.decompose(x, b, k, dref.GADGET)
        assert np.array_equal(lfp.gadget_decompose(x, b, k), want), (b, k)
        assert np.array_equal(plus.gadget_decompose(x, b, k), want), (b, k)
        planes = dref.decompose(x, b, k, dref.PLANES)
        assert np.array_equal(planes.reshape(k, -1, D).transpose(1, 0, 2).reshape(-1, D), want)
        for v in x.reshape(-1):                                                 # every digit is balanced; a tie keeps the sign of the value
            dg, _ = dref.digits(int(v), b, k)
            assert all(abs(d) <= b // 2 for d in dg)
        if b % 2 == 0:
            assert dref.digits(b // 2, b, 2)[0] == [b // 2, 0] and dref.digits(P - b // 2, b, 2)[0] == [-(b // 2), 0]


@pytest.mark.parametrize("b", dref.BASES)
def test_recompose_inverts_decompose_on_what_fits(b):
    for k in dref.DIGITS:
        x = np.array(dref.corner_values(b, k) + [0] * (-len(dref.corner_values(b, k)) % D), dtype=np.uint64).reshape(-1, D)
        for layout in (dref.GADGET, dref.PLANES):
            back = dref.recompose(dref.decompose(x, b, k, layout), b, k, layout)
            for v, w in zip(x.reshape(-1), back.reshape(-1)):
                dg, rest = dref.digits(int(v), b, k)
                assert sum(d * b**i for i, d in enumerate(dg)) + rest * b**k == dref.centre(int(v))
                assert int(w) == (dref.centre(int(v)) - rest * b**k) % P        # the value minus its lost remainder
                if rest == 0:
                    assert int(w) == int(v)
                if b % 2:                                                       # an odd base: it fits exactly when it lies in the balanced range of k digits
                    assert (rest == 0) == (abs(dref.centre(int(v))) <= (b**k - 1) // 2)
            assert np.array_equal(back, dref.kept(x, b, k))


def test_the_gadget_form_of_a_matrix_is_the_host_built_one():
    import lfplus_mlsumcheck_ref as ref
    for b, k, rows, m in ((2, 1, 5, 6), (3, 4, 6, 6), (2**31, 2, 3, 5), (2**62, 3, 4, 4)):
        rp = np.array([0] + sorted(int(x) % 9 for x in dref.rand_words(b % 97 + k, rows - 1)) + [8], dtype=np.uint32)
        col = np.array([int(x) % m for x in dref.rand_words(7 * k, 8)], dtype=np.uint32)
        val = ref.rand_ring(0x90 + k, (8, D))
        n = m * k + 0
        want = plus.pad_rows(plus.gadget_decompose_csr((rp, col, val), b, k), n)
        got = dref.gadget_csr((rp, col, val), b, k, n)
        assert all(np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w) for g, w in zip(got, want)), (b, k)
