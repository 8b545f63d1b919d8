"""Device-memory twins of the LatticeFold+ ABI (include/lfplus.h "device-resident callers") without a GPU: each of the eight twins is declared with the
parameter list of its call, exported by liblfhip.so, listed by plus.exported_symbols(), bound exactly once by the -sys crate and present in the `extern "C"`
block of INTEGRATION.md, as are the two wait_stream calls; a NULL context or prover is LFPLUS_E_ARG on each and touches no buffer; the family adds no lf_*
symbol and leaves the ABI version alone."""
import ctypes as C
import os
import re

import numpy as np

from latticefold_amd import api, plus

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TWINS = ("lfplus_set_witness_dev", "lfplus_witness_from_z_dev", "lfplus_commit_dev", "lfplus_get_witness_dev", "lfplus_decompose_dev",
         "lfplus_prover_ingest_dev", "lfplus_prover_set_instances_dev", "lfplus_prover_accumulator_dev")
ORDERING = ("lfplus_ctx_wait_stream", "lfplus_prover_wait_stream")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfplus.h")).read(), flags=re.S)


def test_header_declares_each_twin_with_the_parameter_list_of_its_call():
    hdr = _header()
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)).strip()
    for s in TWINS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert sig(s) == sig(s[:-4]), s
    assert sig("lfplus_ctx_wait_stream") == "lfplus_ctx *ctx, void *hip_stream"
    assert sig("lfplus_prover_wait_stream") == "lfplus_prover *prover, void *hip_stream"
    # scope: no twin for the commitment matrix, the from_f results, the digit arrays or the relation checks
    for s in ("lfplus_set_matrix_dev", "lfplus_prover_create_dev", "lfplus_rg_read_dev", "lfplus_set_check_dev", "lfplus_range_check_dev", "lfplus_r1cs_check_dev",
              "lfplus_linb_check_dev"):
        assert s not in hdr


def test_each_entry_point_is_exported_listed_and_bound_once():
    lib = plus._nlib()
    listed = plus.exported_symbols()
    sys_crate = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in TWINS + ORDERING:
        assert s in listed, s
        assert hasattr(lib, s), s
        assert len(re.findall(r"pub fn " + s + r"\(", sys_crate)) == 1, s
        assert re.search(r"pub fn " + s + r"\(", doc), s
    assert sorted(n for n in listed if n.endswith("_dev")) == sorted(TWINS)
    assert sum(n.endswith("_dev") for n in listed) == 8


def test_the_family_adds_no_lf_symbol_and_keeps_the_abi_version():
    assert api.abi_version() == 6
    assert sum(n.endswith("_dev") for n in api.exported_symbols()) == 23
    assert not any(n.startswith("lfplus") for n in api.exported_symbols())


def test_null_context_or_prover_is_e_arg_and_touches_nothing():
    L = plus._nlib()
    buf = np.full((4, 16), 7, dtype=np.uint64)
    out = np.full((4, 16), 9, dtype=np.uint64)
    p, po = C.c_void_p(buf.ctypes.data), out.ctypes.data_as(plus.u64p)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data)
    cms = (plus.u64p * 1)(out.ctypes.data_as(plus.u64p))
    assert L.lfplus_ctx_wait_stream(None, None) == plus.E_ARG
    assert L.lfplus_set_witness_dev(None, p, 4) == plus.E_ARG
    assert L.lfplus_witness_from_z_dev(None, p, 4, 2, 1, po) == plus.E_ARG
    assert L.lfplus_commit_dev(None, p, 4, po) == plus.E_ARG
    assert L.lfplus_get_witness_dev(None, p, 4) == plus.E_ARG
    assert L.lfplus_decompose_dev(None, 4, po, po, 0, None, None, None, p, p, po, po, po, po) == plus.E_ARG
    assert L.lfplus_prover_wait_stream(None, None) == plus.E_ARG
    assert L.lfplus_prover_ingest_dev(None, ptrs, 1, 4, 1, po) == plus.E_ARG
    assert L.lfplus_prover_set_instances_dev(None, ptrs, cms, 1) == plus.E_ARG
    assert L.lfplus_prover_accumulator_dev(None, p, p) == plus.E_ARG
    assert (buf == 7).all() and (out == 9).all()
