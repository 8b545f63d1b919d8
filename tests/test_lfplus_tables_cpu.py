"""MLE tables on arrays (lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t and their _device forms) without a GPU: the eight
entry points in header, library, Python mirror and the two Rust crates; one parameter list per pair; the answer to a NULL context; and the Python-integer
references of tests/test_gpu_lfplus_tables.py (tests/lfplus_tables_ref.py) against the definitions they restate."""
import ctypes as C
import os
import re

import numpy as np

import lfplus_mlsumcheck_ref as ref
import lfplus_tables_ref as tref
from latticefold_amd import api, plus

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PAIRS = [("lfplus_build_eq", "lfplus_build_eq_device"), ("lfplus_mle_eval_batch", "lfplus_mle_eval_batch_device"),
         ("lfplus_mle_fix_variables", "lfplus_mle_fix_variables_device"), ("lfplus_spmv_t", "lfplus_spmv_t_device")]
SYMBOLS = [s for pair in PAIRS for s in pair]
P, D = plus.P, plus.D
u64p = plus.u64p
SENT = 0x5A5A5A5A5A5A5A5A


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfplus.h")).read(), flags=re.S)


def _params(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, f"include/lfplus.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_eight_symbols_through_every_layer():
    hdr = _header()
    names = plus.exported_symbols()
    lib = plus._lib()
    nm = os.popen("nm -D --defined-only '%s'" % os.path.join(ROOT, "latticefold_amd", "liblfhip.so")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "plus.rs")).read()
    for s in SYMBOLS:
        params = _params(hdr, s)
        assert s in names, f"plus.exported_symbols() does not list {s}"
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), f"nm -D of liblfhip.so does not show {s}"
        f = getattr(lib, s)
        assert f.argtypes is not None and len(f.argtypes) == len(params), f"{s} has no ctypes prototype of {len(params)} parameters"
        assert sys_rs.count(f"pub fn {s}(") == 1, f"{s} is not bound exactly once in latticefold-hip-sys"
        assert f"pub fn {s}(" in integ, f"INTEGRATION.md does not list {s}"
        assert f"sys::{s}(" in safe, f"the safe crate does not call {s}"
        assert f"pub fn {s[len('lfplus_'):]}(" in safe or f"pub unsafe fn {s[len('lfplus_'):]}(" in safe, f"the safe crate has no wrapper named after {s}"
    for host, device in PAIRS:                                                  # device and host form: one parameter list
        assert _params(hdr, host) == _params(hdr, device)
    assert all(hasattr(plus.PlusContext, n) for n in ("build_eq", "mle_eval_batch", "mle_fix_variables", "spmv_t"))


def test_the_section_sits_behind_the_ring_arithmetic_and_naming_stays():
    hdr = open(os.path.join(ROOT, "include", "lfplus.h")).read()
    assert hdr.index("ring arithmetic on arrays:") < hdr.index("MLE tables on arrays:") < hdr.index("committed CCS instances:")
    assert hdr.index("int lfplus_spmv_device(") < hdr.index("int lfplus_build_eq(")
    assert not any(s.endswith("_dev") for s in SYMBOLS)
    assert len([s for s in plus.exported_symbols() if s.endswith("_dev")]) == 8
    assert api.abi_version() == 6


def test_a_null_context_is_refused_before_any_device_is_touched():
    lib = plus._lib()
    t, out = (np.full((4, D), SENT, dtype=np.uint64) for _ in range(2))
    pt = np.full(2, SENT, dtype=np.uint64)
    pt_, po, pp = t.ctypes.data_as(u64p), out.ctypes.data_as(u64p), pt.ctypes.data_as(u64p)
    vt, vo = C.c_void_p(t.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.lfplus_build_eq(None, pp, 2, po) == plus.E_ARG
    assert lib.lfplus_build_eq_device(None, pp, 2, vo) == plus.E_ARG
    assert lib.lfplus_mle_eval_batch(None, pt_, 1, 4, pp, 2, po) == plus.E_ARG
    assert lib.lfplus_mle_eval_batch_device(None, vt, 1, 4, pp, 2, po) == plus.E_ARG
    assert lib.lfplus_mle_fix_variables(None, pt_, 1, 4, pp, 1, po) == plus.E_ARG
    assert lib.lfplus_mle_fix_variables_device(None, vt, 1, 4, pp, 1, vo) == plus.E_ARG
    assert lib.lfplus_spmv_t(None, 0, pt_, 4, po) == plus.E_ARG
    assert lib.lfplus_spmv_t_device(None, 0, vt, 4, vo) == plus.E_ARG
    assert all((x == SENT).all() for x in (t, out, pt)), "the buffers are untouched"


def test_the_references_agree_with_the_definitions_they_restate():
    """eq by the product formula is the eq_table the sumcheck tests build level by level; an evaluation is the table fixed variable by variable
    (lfplus_mlsumcheck_ref.fix); the transposed loop is the adjoint of the row loop"""
    r = [0, 1, P - 1, int(ref.rand_ring(0x31, (1,))[0])]
    assert np.array_equal(tref.eq_words(r), ref.eq_table(r)[:, 0])
    tables = ref.rand_ring(0x32, (3, 16, D))
    cur = tables.astype(object)
    for ri in r:
        cur = ref.fix(cur, ri)
    assert np.array_equal(tref.py_eval(tables, 16, r), (cur[:, 0] % P).astype(np.uint64))
    assert np.array_equal(tref.py_fix(tables, r[:1]), (ref.fix(tables.astype(object), r[0]) % P).astype(np.uint64))
    ragged = tables.copy()
    ragged[:, 11:] = 0
    assert np.array_equal(tref.py_eval(np.ascontiguousarray(tables[:, :11]), 11, r), tref.py_eval(ragged, 16, r))
    n = 8
    mat = ref.rand_csr(0x33, n, 2)
    x, v = ref.rand_ring(0x34, (n, D)), ref.rand_ring(0x35, (n, D))
    lhs = ref.rmul(ref.spmv(mat, x), v).sum(axis=0) % P
    rhs = ref.rmul(x, tref.py_spmv_t(mat, v)).sum(axis=0) % P
    assert np.array_equal(lhs, rhs)
