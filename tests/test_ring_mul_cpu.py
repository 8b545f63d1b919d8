"""lf_ring_mul and its device-memory form lf_ring_mul_device without a GPU: declared by include/lfhip.h with one parameter list, exported by liblfhip.so, listed
by api.exported_symbols(), prototyped for ctypes with seven arguments each, bound by the -sys crate, by the `extern "C"` block of INTEGRATION.md and by the safe
crate; a NULL context or a bad argument is LF_ERR_INVALID before any device is touched; without a GPU there is no context, so the wrapper ends in LF_ERR_HIP.
The references of the GPU tests (tests/test_gpu_ring_mul.py) are checked against each other and against the oracle's CRT here, where no GPU is needed."""
import os
import re

import numpy as np
import pytest

from latticefold_amd import api
from latticefold_amd.workload import RINGS, ring_mul_ntt

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMS = ("lf_ring_mul", "lf_ring_mul_device")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfhip.h")).read(), flags=re.S)


def test_both_symbols_are_declared_exported_listed_and_bound():
    hdr, lib, listed = _header(), api._lib(), api.exported_symbols()
    sys_crate = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    safe_crate = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)).strip()
    for s in SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert s in listed and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == 7, s
        assert len(re.findall(r"pub fn " + s + r"\(", sys_crate)) == 1, s
        assert re.search(r"pub fn " + s + r"\(", doc), s
        assert "sys::" + s + "(" in safe_crate, s
    assert sig(SYMS[0]) == sig(SYMS[1])
    assert re.search(r"#define LF_FORM_NTT\s+0\b", hdr) and re.search(r"#define LF_FORM_COEFF\s+1\b", hdr)
    assert api.FORMS == {"ntt": 0, "coeff": 1}
    assert "pub const LF_FORM_NTT: c_int = 0;" in sys_crate and "pub const LF_FORM_COEFF: c_int = 1;" in sys_crate
    assert len(listed) == 125


def test_bad_arguments_are_invalid_without_a_device():
    L = api._lib()
    buf = np.zeros((4, 24), dtype=np.uint64)
    p, pp = buf.ctypes.data, buf.ctypes.data_as(api.u64p)
    for form in (0, 1):
        assert L.lf_ring_mul(None, pp, pp, 1, 4, form, pp) == -1 and L.lf_ring_mul_device(None, p, p, 1, 4, form, p) == -1
    assert not buf.any()


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a = np.zeros((4, 24), dtype=np.uint64)
    for ring in ("goldilocks", "babybear"):
        with pytest.raises(api.LfError) as e:
            api.Context(0, ring=ring).ring_mul(a, a)
        assert e.value.code == -2   # LF_ERR_HIP


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_the_two_references_agree_through_the_oracle_crt(ring):
    """crt(a . b) == ring_mul_ntt(crt a, crt b), a . b the big-integer product mod the cyclotomic polynomial: rows of p - 1, the unit and random rows"""
    from ring_mul_refs import coeff_sum_bigint
    if ring == "goldilocks":
        import lfo as O
    else:
        import lfo_bb as O
    p, d, _tau = RINGS[ring]
    rng = np.random.default_rng(5)
    a = np.stack([np.full(d, p - 1, dtype=np.uint64), np.eye(1, d, dtype=np.uint64)[0], rng.integers(0, p, d, dtype=np.uint64), rng.integers(0, p, d, dtype=np.uint64)])
    b = np.stack([np.full(d, p - 1, dtype=np.uint64), rng.integers(0, p, d, dtype=np.uint64), rng.integers(0, p, d, dtype=np.uint64), np.full(d, (p + 1) // 2, dtype=np.uint64)])
    prod = coeff_sum_bigint(a[None], b[None], ring)
    assert (prod[1] == b[1]).all()
    assert (O.crt(prod) == ring_mul_ntt(O.crt(a), O.crt(b), ring)).all()
