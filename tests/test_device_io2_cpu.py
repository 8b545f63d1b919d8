"""Device-memory twins of the component calls (decompose, recompose, linf_check, build_eq, mle_eval_batch, spmv, the two sumcheck begins, lincomb,
horner_combine) without a GPU: each is declared by include/lfhip.h with the parameter list of its twin, exported by liblfhip.so, listed by
api.exported_symbols(), bound by the -sys crate and by the `extern "C"` block of INTEGRATION.md; a NULL context is LF_ERR_INVALID on each; the ABI version stays
the one that numbers the _dev family."""
import ctypes as C
import os
import re

import numpy as np

from latticefold_amd import api

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
DEV_SYMS = ("lf_decompose_dev", "lf_recompose_dev", "lf_linf_check_dev", "lf_build_eq_dev", "lf_mle_eval_batch_dev", "lf_spmv_dev",
            "lf_sumcheck_lin_begin_dev", "lf_sumcheck_fold_begin_dev", "lf_lincomb_dev", "lf_horner_combine_dev")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfhip.h")).read(), flags=re.S)


def test_header_declares_each_twin_with_the_signature_of_its_call():
    hdr = _header()
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)).strip()
    for s in DEV_SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert sig(s) == sig(s[:-4]), s
    # the _round and _end calls of the sumchecks take O(1) arguments: no twin
    for s in ("lf_sumcheck_lin_round_dev", "lf_sumcheck_lin_end_dev", "lf_sumcheck_fold_round_dev", "lf_sumcheck_fold_end_dev"):
        assert s not in hdr


def test_each_twin_is_exported_listed_and_bound():
    lib = api._lib()
    listed = api.exported_symbols()
    sys_crate = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in DEV_SYMS:
        assert s in listed, s
        assert hasattr(lib, s), s
        assert len(re.findall(r"pub fn " + s + r"\(", sys_crate)) == 1, s
        assert re.search(r"pub fn " + s + r"\(", doc), s
    assert sum(n.endswith("_dev") for n in listed) == 23


def test_abi_version_is_unchanged():
    assert api.abi_version() == 6


def test_null_context_is_invalid_on_each_twin():
    L = api._lib()
    buf = np.zeros((4, 24), dtype=np.uint64)
    p, pp = buf.ctypes.data, buf.ctypes.data_as(api.u64p)
    ok = C.c_int(7)
    assert L.lf_decompose_dev(None, p, 2, 4, 2, 0, p) == -1
    assert L.lf_recompose_dev(None, p, 2, 4, 2, p) == -1
    assert L.lf_linf_check_dev(None, p, 4, 8, 0, C.byref(ok), pp) == -1 and ok.value == 7
    assert L.lf_build_eq_dev(None, pp, 2, p) == -1
    assert L.lf_mle_eval_batch_dev(None, p, 1, 4, pp, 2, pp) == -1
    assert L.lf_spmv_dev(None, 0, p, p) == -1
    assert L.lf_sumcheck_lin_begin_dev(None, p, pp) == -1
    assert L.lf_sumcheck_fold_begin_dev(None, p, pp) == -1
    assert L.lf_lincomb_dev(None, pp, p, 1, 4, p) == -1
    assert L.lf_horner_combine_dev(None, p, 1, 1, 4, pp, p) == -1
    assert not buf.any()
