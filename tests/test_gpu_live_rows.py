"""Skipping the trailing empty rows of the constraint matrices (csrc/lf_live_rows.h): M z, the linearization rounds and the G tables of fold prepare over the
live rows only, word for word against the CPU oracle and against the whole-table launches (LF_NO_LIVE_ROWS).

The CCS of a workload is rearranged after make_workload: entry k of every matrix (column k, the same values) moves to a chosen row, so the last non-empty row
sits where a case wants it and the instance stays satisfied (row r of A, B, C still refers to one variable: z_k * z_k = z_k * z_k).  LF_LIVE_ROWS_LOW lowers the
size threshold and the granule (8 rows) and LF_TAIL_N the persistent tail's size, so that at m = 2^10 / 2^12 several rounds run on the live prefix, the rest is
zero-filled once and the tail takes whole tables."""
import ctypes as C

import numpy as np
import pytest

import lfo
from fold_paths import LIVE_LOW as LOW, LIVE_OFF, LIVE_SPLIT as SPLIT, LIVE_TAIL_N as TAIL_N     # LF_LIVE_ROWS_LOW + LF_TAIL_N = 64; ... + LF_LIN_SPLIT_MIN = 16
from latticefold_amd import api
from latticefold_amd.workload import make_workload

pytestmark = pytest.mark.gpu

G = 8   # granule under LF_LIVE_ROWS_LOW


def _place(wl, pos):
    """entries 0 .. len(pos)-1 of every matrix to the rows `pos` (increasing), one per row; all other rows empty"""
    pos = np.asarray(pos, dtype=np.int64)
    assert (np.diff(pos) > 0).all() and (len(pos) == 0 or (pos[0] >= 0 and pos[-1] < wl.m))
    rp = np.searchsorted(pos, np.arange(wl.m + 1), side="left").astype(np.uint32)   # rowptr[r] = entries in rows < r
    for j in range(wl.t):
        assert len(wl.col[j]) >= len(pos) and len(wl.col[j]) == int(wl.rowptr[j][-1])   # (one entry per row as built)
        wl.rowptr[j] = rp.copy()
        wl.col[j] = np.ascontiguousarray(wl.col[j][:len(pos)])
        wl.val[j] = np.ascontiguousarray(wl.val[j][:len(pos)])
    return wl


def _last_at(wl, last):
    """rows 0 .. last all non-empty while the system has entries for them, the last entry at row `last` in any case"""
    rows = min(wl.n, wl.m)
    return _place(wl, np.arange(last + 1) if last < rows else np.concatenate([np.arange(rows - 1), [last]]))


def _build(name, ccs, kind):
    wl = make_workload(name, ccs=ccs)
    if kind == "asbuilt":
        return wl
    if kind == "empty":
        return _place(wl, [])
    if kind == "gaps":      # row 0 empty, runs of empty rows in the middle; the last entry at row 1 + 3 * 49 = 148
        return _place(wl, 1 + 3 * np.arange(50))
    return _last_at(wl, int(kind))


# (workload, ccs, rows, environment)
CASES = [("T10", "r1cs", str(r), LOW) for r in (0, 1, 2, 3, 5, G - 1, G, G + 1, 127, 1024 // 2 - 1, 1024 // 2, 1024 - 1)]
CASES += [("T10", "r1cs", "gaps", LOW), ("T10", "r1cs", "empty", LOW), ("T10", "r1cs", "asbuilt", LOW), ("T10", "r1cs", "127", SPLIT),
          ("T10", "deg3", "127", LOW), ("T8", "deg5", "31", LOW), ("T12", "r1cs", "767", LOW), ("T12", "r1cs", "767", SPLIT)]
IDS = [f"{n}-{c}-{k}-{'split' if e is SPLIT else 'low'}" for n, c, k, e in CASES]

_refs = {}


def _reference(name, ccs, kind):
    """the workload and the oracle's linearization and fold step, computed once per (workload, ccs, rows) and left unchanged"""
    key = (name, ccs, kind)
    if key not in _refs:
        wl = _build(name, ccs, kind)
        inst = lfo.Instance(wl)
        f = inst.witness_from_w_ccs(wl.w_ccs)
        _refs[key] = (wl, inst, f, {})
    return _refs[key]


def _oracle(ref, cccs, A):
    wl, inst, f, out = ref
    if not out:
        out["acc"], out["lin"] = inst.linearize(lfo.Transcript(), cccs, f)
        out["lc"], out["f0"], out["proof"] = inst.fold_step(lfo.Transcript(), A, out["acc"], f, cccs, f)
    return out


def _numpy_live_rows(wl):
    live = 0
    for rp in wl.rowptr:
        nz = np.nonzero(np.diff(np.asarray(rp, dtype=np.int64)))[0]
        if len(nz):
            live = max(live, int(nz[-1]) + 1)
    return live


def _expected_live_rounds(wl, live, low, tail_n):
    """the schedule of lf_live_rows.h cut where the driver wants whole tables: the persistent tail (not for the wide kernel) and previous tables below 8 entries"""
    L = api._lib()
    L.lfdbg_live_schedule.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_uint, C.POINTER(C.c_size_t)]
    L.lfdbg_live_schedule.restype = None
    e = (C.c_size_t * wl.s)()
    L.lfdbg_live_schedule(wl.m, live, 1 if low else 0, wl.s, e)
    wide = wl.t > 4 or wl.d > 3
    cnt, alive = 0, True
    for r in range(1, wl.s + 1):
        n = wl.m >> (r - 1)
        if r >= 2 and ((not wide and 4 <= 2 * n <= tail_n) or 2 * n < 8):
            alive = False
        alive = alive and e[r - 1] < n
        cnt += alive
    return cnt


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _run(wl, env, monkeypatch):
    for k in ("LF_LIVE_ROWS_LOW", "LF_TAIL_N", "LF_LIN_SPLIT_MIN", "LF_NO_LIVE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = api.Context(0)
    try:
        ctx.load_ccs(wl)
        A = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        acc, lin = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
        live_rounds = ctx.lin_live_rounds()
        lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, api.PoseidonTranscript())
        return {"acc": acc, "lin": lin, "lc": lc, "f0": np.array(w0.f), "proof": proof, "cccs": cccs, "A": A, "live_rows": ctx.live_rows(), "live_rounds": live_rounds}
    finally:
        ctx.close()


@pytest.mark.parametrize("name,ccs,kind,env", CASES, ids=IDS)
def test_live_rows_match_the_oracle_and_the_whole_tables(name, ccs, kind, env, monkeypatch):
    ref = _reference(name, ccs, kind)
    wl = ref[0]
    on = _run(wl, env, monkeypatch)
    off = _run(wl, dict(env, **LIVE_OFF), monkeypatch)
    want = _oracle(ref, on["cccs"], on["A"])
    # the count lf_ccs_load keeps, and the rounds that really ran on a prefix
    live = _numpy_live_rows(wl)
    assert on["live_rows"] == live and off["live_rows"] == live
    if kind.isdigit():
        assert live == int(kind) + 1
    assert on["live_rounds"] == _expected_live_rounds(wl, live, True, TAIL_N)
    assert off["live_rounds"] == 0
    if kind in ("127", "767"):
        assert on["live_rounds"] >= 5
    for key, what in (("lin", "linearization proof"), ("acc", "LCCCS"), ("proof", "fold-step proof"), ("lc", "folded LCCCS"), ("f0", "folded witness")):
        _same(on[key], want[key], f"{what} vs the oracle")
        _same(off[key], on[key], f"{what}: LF_NO_LIVE_ROWS vs the live rows")
    if kind == "empty":     # every M_j z is zero: so is every message of the linearization sumcheck
        assert not np.asarray(on["lin"]).reshape(-1)[: wl.s * (wl.d + 2) * 24].any()


def test_default_threshold_keeps_small_shapes_whole(monkeypatch):
    """without LF_LIVE_ROWS_LOW a system of 2^10 rows is below the size from which the prefix is used: every round runs whole (and the proof is the oracle's)"""
    ref = _reference("T10", "r1cs", "127")
    wl = ref[0]
    got = _run(wl, {}, monkeypatch)
    assert got["live_rows"] == 128 and got["live_rounds"] == 0
    want = _oracle(ref, got["cccs"], got["A"])
    for key in ("lin", "acc", "proof", "lc", "f0"):
        _same(got[key], want[key], key)
