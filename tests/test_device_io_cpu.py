"""Device-resident callers without a GPU: the `_dev` entry points and lf_ctx_wait_stream are declared by include/lfhip.h, exported by liblfhip.so and listed by
api.exported_symbols(); the ABI version is the one that numbers them; and without a GPU every path to them ends in LF_ERR_HIP (no context can be made, there is
no host fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from latticefold_amd import api

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
DEV_SYMS = ("lf_ntt_fwd_dev", "lf_ntt_inv_dev", "lf_ajtai_commit_dev", "lf_ajtai_commit_coeff_dev", "lf_ajtai_decompose_and_commit_coeff_dev",
            "lf_ajtai_decompose_and_commit_ntt_dev", "lf_witness_from_w_ccs_dev", "lf_witness_from_f_coeff_dev", "lf_witness_from_f_dev",
            "lf_witness_get_f_dev", "lf_witness_get_f_coeff_dev", "lf_witness_get_w_ccs_dev", "lf_ccs_check_dev")
SYMS = DEV_SYMS + ("lf_ctx_wait_stream",)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfhip.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_device_entry_points():
    hdr = _header()
    lib = api._lib()
    listed = api.exported_symbols()
    for s in SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert s in listed, s
        assert hasattr(lib, s), s
    # every twin has the signature of the call it mirrors
    for s in DEV_SYMS:
        sig = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)).strip()
        assert sig(s) == sig(s[:-4]), s


def test_abi_version_numbers_the_device_entry_points():
    assert api.abi_version() == 6
    assert int(re.search(r"#define LFHIP_ABI_VERSION (\d+)", _header()).group(1)) == 6


def test_null_context_is_invalid_and_no_gpu_is_lf_err_hip():
    """a NULL context is LF_ERR_INVALID on every symbol, as on their twins; without a GPU no context exists, so every wrapper ends in LF_ERR_HIP"""
    import torch
    L = api._lib()
    buf = np.zeros((4, 24), dtype=np.uint64)
    p, h = buf.ctypes.data, C.c_void_p()
    pp = buf.ctypes.data_as(api.u64p)
    assert L.lf_ctx_wait_stream(None, None) == -1
    assert L.lf_ntt_fwd_dev(None, p, p, 4) == -1 and L.lf_ntt_inv_dev(None, p, p, 4) == -1
    assert L.lf_ajtai_commit_dev(None, p, 4, 1, pp) == -1 and L.lf_ajtai_commit_coeff_dev(None, p, 4, 1, pp) == -1
    assert L.lf_ajtai_decompose_and_commit_coeff_dev(None, p, 2, 4, 2, 1, pp) == -1
    assert L.lf_ajtai_decompose_and_commit_ntt_dev(None, p, 2, 4, 2, 1, pp) == -1
    for f in (L.lf_witness_from_w_ccs_dev, L.lf_witness_from_f_coeff_dev, L.lf_witness_from_f_dev):
        assert f(None, p, C.byref(h)) == -1 and not h.value
    for f in (L.lf_witness_get_f_dev, L.lf_witness_get_f_coeff_dev, L.lf_witness_get_w_ccs_dev):
        assert f(None, None, p) == -1
    assert L.lf_ccs_check_dev(None, p, pp) == -1
    assert not buf.any()
    if torch.cuda.is_available():
        return
    for ring in ("goldilocks", "babybear"):
        with pytest.raises(api.LfError) as e:
            api.Context(0, ring=ring).ntt_fwd(buf)
        assert e.value.code == -2   # LF_ERR_HIP


def test_device_arrays_are_recognised_by_duck_type():
    class Fake:
        is_cuda = True

        def data_ptr(self):
            return 0

    class HostFake(Fake):
        is_cuda = False

    assert api.is_device_array(Fake()) and not api.is_device_array(HostFake()) and not api.is_device_array(np.zeros(3))
    import torch
    assert not api.is_device_array(torch.zeros(3))
