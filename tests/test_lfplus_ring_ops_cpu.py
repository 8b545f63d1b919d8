"""Ring arithmetic on arrays (lfplus_ring_mul, lfplus_spmv and their _device forms) without a GPU: the four entry points in header, library, Python mirror and
the two Rust crates; the mode constants; the answer to a NULL context; and the two references of tests/test_gpu_lfplus_ring_ops.py -- the Python-integer product
of tests/lfplus_mlsumcheck_ref.py and the oracle's lfp_ring_mul -- against each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfp
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import api, plus

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMBOLS = ["lfplus_ring_mul", "lfplus_ring_mul_device", "lfplus_spmv", "lfplus_spmv_device"]
P, D = plus.P, plus.D
u64p = plus.u64p
SENT = 0x5A5A5A5A5A5A5A5A


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfplus.h")).read(), flags=re.S)


def _params(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, f"include/lfplus.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_four_symbols_through_every_layer():
    hdr = _header()
    names = plus.exported_symbols()
    lib = plus._lib()
    sys_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "plus.rs")).read()
    for s in SYMBOLS:
        params = _params(hdr, s)
        assert s in names, f"plus.exported_symbols() does not list {s}"
        assert hasattr(lib, s), f"liblfhip.so does not export {s}"
        f = getattr(lib, s)
        assert f.argtypes is not None and len(f.argtypes) == len(params), f"{s} has no ctypes prototype of {len(params)} parameters"
        assert sys_rs.count(f"pub fn {s}(") == 1, f"{s} is not bound exactly once in latticefold-hip-sys"
        assert f"pub fn {s}(" in integ, f"INTEGRATION.md does not list {s}"
        assert f"sys::{s}(" in safe, f"the safe crate does not call {s}"
    # device and host form: one parameter list
    assert _params(hdr, "lfplus_ring_mul") == _params(hdr, "lfplus_ring_mul_device")
    assert _params(hdr, "lfplus_spmv") == _params(hdr, "lfplus_spmv_device")
    assert all(hasattr(plus.PlusContext, n) for n in ("ring_mul", "spmv"))


def test_mode_constants_agree():
    hdr = _header()
    sys_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    for name, mine in (("LFPLUS_MUL_ELEMENTWISE", plus.MUL_ELEMENTWISE), ("LFPLUS_MUL_BROADCAST", plus.MUL_BROADCAST)):
        h = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        r = re.search(r"pub const %s: c_int = (\d+);" % name, sys_rs)
        assert h and r and int(h.group(1)) == int(r.group(1)) == mine
    assert (plus.MUL_ELEMENTWISE, plus.MUL_BROADCAST) == (0, 1)


def test_naming_and_abi_version():
    """the device forms are spelled _device: the _dev families keep their size, the ABI version stays"""
    assert not any(s.endswith("_dev") for s in SYMBOLS)
    assert len([s for s in plus.exported_symbols() if s.endswith("_dev")]) == 8
    assert api.abi_version() == 6


def test_a_null_context_is_refused_before_any_device_is_touched():
    lib = plus._lib()
    a, b, out = (np.full((2, D), SENT, dtype=np.uint64) for _ in range(3))
    pa, pb, po = (x.ctypes.data_as(u64p) for x in (a, b, out))
    va, vb, vo = (C.c_void_p(x.ctypes.data) for x in (a, b, out))
    for mode in (0, 1):
        assert lib.lfplus_ring_mul(None, pa, pb, 1, 2, mode, po) == plus.E_ARG
        assert lib.lfplus_ring_mul_device(None, va, vb, 1, 2, mode, vo) == plus.E_ARG
    assert lib.lfplus_spmv(None, 0, pa, 2, po) == plus.E_ARG
    assert lib.lfplus_spmv_device(None, 0, va, 2, vo) == plus.E_ARG
    assert all((x == SENT).all() for x in (a, b, out)), "the buffers are untouched"


def _oracle_rows(a, b):
    return np.stack([lfp.ring_mul(x, y) for x, y in zip(a, b)])


def test_the_two_references_agree():
    full = np.full((1, D), P - 1, dtype=np.uint64)
    one = np.zeros((1, D), dtype=np.uint64)
    one[0, 0] = 1
    x15 = np.zeros((1, D), dtype=np.uint64)
    x15[0, 15] = 1
    rnd = ref.rand_ring(0x91, (6, D))
    a = np.concatenate([full, full, one, x15, rnd])
    b = np.concatenate([full, one, ref.rand_ring(0x92, (1, D)), x15, ref.rand_ring(0x93, (6, D))])
    got = ref.rmul(a, b).astype(np.uint64)
    assert np.array_equal(got, _oracle_rows(a, b))
    # the wrap sign: X^15 X^15 = X^30 = -X^14; the unit is neutral
    want = np.zeros(D, dtype=np.uint64)
    want[14] = P - 1
    assert np.array_equal(got[3], want) and np.array_equal(got[2], b[2])
