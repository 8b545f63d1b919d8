"""The witness tables of include/lfhip_tables.h without a GPU: the ten symbols in header, library, generated binding and Python surface, and the numpy
restatements tests/test_gpu_witness_tables.py compares the device against (tests/witness_tables_ref.py), held to the CPU oracle:

  f-hat by formula     tab_j[:N, 0::tau] = f_coeff[:, 8j:8j+8] evaluates to v_j of the oracle's LCCCS at its point r
  M z and M^T v        <M_j z, eq(r)> = u_j = <z, M_j^T eq(r)> from the same LCCCS (layout r[s] v[tau] cm[kappa] u[t] ..)
  fix                  the numpy fix applied s times is lfo.mle_eval
at T8, G5 (N 320 < m 512: the zero tail), B6 and B333 (tau 9, N 666 < m 1024)."""
import importlib.util
import os
import re

import numpy as np
import pytest

from latticefold_amd import api
from latticefold_amd.workload import make_workload
from witness_tables_ref import (NEW_SYMBOLS, SPMV_T_CHUNK, SPMV_T_HEAVY, csr_from_columns, embed, fhat_np, fix_np, inner_np, lcccs_parts, oracle_for, rand_ring,
                                spmv_np, spmv_t_np)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_header_library_and_binding_agree():
    assert tuple(api.exported_symbols("lfhip_tables.h")) == tuple(sorted(NEW_SYMBOLS))
    assert all(hasattr(api._lib(), s) for s in NEW_SYMBOLS)
    assert not [s for s in NEW_SYMBOLS if s.endswith("_dev")]          # the _dev names of lfhip.h are a counted set: the twins here end in _device
    assert not set(NEW_SYMBOLS) & set(api.exported_symbols())          # declared in the included file, not in lfhip.h itself
    main = open(os.path.join(ROOT, "include", "lfhip.h")).read()
    assert main.index('#include "lfhip_tables.h"') < main.rindex("#ifdef __cplusplus")
    spec = importlib.util.spec_from_file_location("gen_rust_bindings", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text, fns = gen.generate_tables()
    assert sorted(fns) == sorted(NEW_SYMBOLS) and len(fns) == len(set(fns)) == 10
    for s in NEW_SYMBOLS:
        assert len(re.findall(r"pub fn " + s + r"\(", text)) == 1, s   # declared once
    assert open(gen.TABLES_OUT).read() == text, "run tools/gen_rust_bindings.py --write"
    doc = open(gen.DOC).read()
    block = doc[doc.index(gen.TABLES_BEGIN) + len(gen.TABLES_BEGIN):doc.index(gen.TABLES_END)]
    assert block.strip() == ("```rust\n" + text + "```").strip(), "run tools/gen_rust_bindings.py --write"
    assert "pub mod tables;" in open(gen.OUT).read()
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read()
    assert set(re.findall(r"sys::tables::(lf_[a-z0-9_]+)\(", safe)) <= set(NEW_SYMBOLS)
    for name in ("f_hat", "z", "mz", "mul_vec_transposed"):
        assert re.search(r"pub fn " + name + r"[<(]", safe), name
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert 'exported_symbols("lfhip_tables.h")' in entry


def test_python_surface_and_kernel_constants():
    for owner, meth in ((api.Witness, "get_fhat"), (api.Witness, "get_z"), (api.Witness, "mz"), (api.Context, "mat_vec_mul_t"), (api, "get_fhat"),
                        (api, "mle_fix_variables")):
        assert callable(getattr(owner, meth))
    plan = open(os.path.join(ROOT, "latticefold_amd", "csrc", "lf_spmv_t_plan.h")).read()
    assert int(re.search(r"SPMV_T_HEAVY = (\d+);", plan).group(1)) == SPMV_T_HEAVY
    assert int(re.search(r"SPMV_T_CHUNK = (\d+);", plan).group(1)) == SPMV_T_CHUNK


@pytest.fixture(scope="module", params=["T8", "G5", "B6", "B333"])
def lin(request):
    """(workload, oracle, f_coeff, r, v, u) of the oracle's linearization of the workload's own instance"""
    wl = make_workload(request.param, 0)
    O = oracle_for(wl.ring)
    inst = O.Instance(wl)
    f = inst.witness_from_w_ccs(wl.w_ccs)
    cccs = np.concatenate([O.ajtai_commit(inst.ajtai_matrix(), wl.kappa, wl.N, O.crt(f)), wl.x_ccs])
    lcccs, _ = inst.linearize(O.Transcript(), cccs, f)
    return (wl, O, f) + lcccs_parts(lcccs, wl)


def test_fhat_formula_reproduces_v(lin):
    wl, O, f, r, v, _ = lin
    tabs = fhat_np(f, wl)
    assert not tabs[:, wl.N:].any() and not np.delete(tabs, np.s_[0::wl.tau], axis=2).any()
    for j in range(wl.tau):
        assert (O.mle_eval(tabs[j], r) == v[j]).all(), (wl.name, j)


def test_mz_and_transposed_product_reproduce_u(lin):
    wl, O, _, r, _, u = lin
    z, eq = wl.z(), O.build_eq(r)
    for j in range(wl.t):
        mz = spmv_np(wl.rowptr[j], wl.col[j], wl.val[j], z, wl.m, wl.ring)
        assert (O.mle_eval(mz, r) == u[j]).all(), (wl.name, j)
        assert (inner_np(mz, eq, wl.ring) == u[j]).all(), (wl.name, j)
        assert (inner_np(z, spmv_t_np(wl.rowptr[j], wl.col[j], wl.val[j], eq, wl.n, wl.ring), wl.ring) == u[j]).all(), (wl.name, j)


def test_numpy_fix_applied_s_times_is_mle_eval(lin):
    wl, O, _, r, _, _ = lin
    tab = rand_ring(0xF1C5 + wl.s, wl.m, wl)
    cur = tab
    for i in range(wl.s):
        assert (r[i] == embed(r[i][:wl.tau])).all()     # the point of an LCCCS is made of slot-constant elements
        cur = fix_np(cur, r[i], wl.ring)
    assert cur.shape == (1, wl.RE) and (cur[0] == O.mle_eval(tab, r)).all()


def test_adjoint_identity_on_a_hand_built_matrix():
    """<M z, v> = <z, M^T v> in numpy on the kind of matrix the GPU test builds: the two restatements agree with each other before the device is held to them"""
    wl = make_workload("T8", 0)
    m, n = 64, 40
    counts = np.zeros(n, dtype=np.int64)
    counts[[1, 2, 7, 30]] = [64, 33, 1, 5]
    rp, ci, va = csr_from_columns(counts, m, n, wl, 3)
    assert rp[-1] == counts.sum() and (np.bincount(ci, minlength=n) == counts).all()
    z, v = rand_ring(4, n, wl), rand_ring(5, m, wl)
    assert (inner_np(spmv_np(rp, ci, va, z, m, wl.ring), v, wl.ring) == inner_np(z, spmv_t_np(rp, ci, va, v, n, wl.ring), wl.ring)).all()
