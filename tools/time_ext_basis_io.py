#!/usr/bin/env python3
"""The O(n) calls of a context in an EXTERNAL basis (lf_set_ext_basis) against the same calls in the default basis, host-pointer and `_dev` spelling, in one
process: wall-clock time of calls that end in the library's own synchronise.  Sibling of tools/time_device_io.py (same shapes, same clock).

    python tools/time_ext_basis_io.py [--reps 9] [--label this] [--out profiles/ext_basis_io_times.jsonl] [--only NAME ...] [--no-dev]

Contexts: Goldilocks with a random basis change T, BabyBear with the tower basis F_{p^3}[Z]/(Z^3 - u) (a permutation), and a default-basis context of the same
ring next to each.  Calls: commit_ntt at the reference's CommitNTT rows (n = 2^20), Witness::from_w_ccs and lf_witness_get_f at C4 (Goldilocks) and C3
(BabyBear).  Per shape the variants ALTERNATE inside every repetition.  One JSON line per shape: min and median in ms of
    xb_host_ptr / xb_dev            the external-basis context
    default_host_ptr / default_dev  the default-basis context (the cost of one relayout pass is the yardstick of the basis change)
--no-dev leaves the `_dev` spellings out (a library from before they accepted external-basis contexts); --label names the library in the rows, so the rows
of two builds can sit in one file (--append)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from latticefold_amd import api  # noqa: E402
from latticefold_amd.workload import RINGS, make_workload, splitmix_fq  # noqa: E402


def dev(a):
    return torch.from_numpy(a.view(np.int64)).to("cuda")


def tower_T(tau=9):
    """external index 3j+i (u^i Z^j, Z^3 = u) <-> internal exponent 3i+j (Y = Z, u = Y^3)"""
    T = np.zeros((tau, tau), dtype=np.uint64)
    for i in range(3):
        for j in range(3):
            T[3 * j + i, 3 * i + j] = 1
    return T


def random_T(ring, seed):
    """a random basis change that fixes 1; lf_set_ext_basis refuses a singular one, so the caller tries the next seed"""
    _p, _d, tau = RINGS[ring]
    T = splitmix_fq(seed, 0, tau * tau, ring).reshape(tau, tau).copy()
    T[:, 0] = 0
    T[0, 0] = 1
    return T


def ext_context(ring):
    ctx = api.Context(0, ring=ring)
    if ring == "babybear":
        ctx.set_ext_basis(tower_T())
        return ctx
    for seed in range(4242, 4250):
        try:
            ctx.set_ext_basis(random_T(ring, seed))
            return ctx
        except api.LfError:
            pass
    raise RuntimeError("no invertible basis")


def measure(calls, reps, warmup):
    for _ in range(warmup):
        for c in calls.values():
            c()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return t


def row(label, name, ring, mbytes, t):
    r = {"library": label, "shape": name, "ring": ring, "array_MB": round(mbytes, 1), "reps": len(next(iter(t.values())))}
    for k, v in t.items():
        r[k + "_ms"] = {"min": round(min(v), 3), "median": round(statistics.median(v), 3)}
    return r


def commit_ntt(a, ring, kappa):
    n = 1 << 20
    xb, plain = ext_context(ring), api.Context(0, ring=ring)
    try:
        sx = api.AjtaiCommitmentScheme(xb, kappa=kappa, n=n, seed=7)
        sp = api.AjtaiCommitmentScheme(plain, kappa=kappa, n=n, seed=7)
        f = splitmix_fq(11, 0, n * xb.RE, ring).reshape(n, xb.RE)
        fd = dev(f)
        torch.cuda.synchronize()
        calls = {"xb_host_ptr": lambda: sx.commit(f), "default_host_ptr": lambda: sp.commit(f)}
        if a.dev:
            calls.update({"xb_dev": lambda: sx.commit(fd), "default_dev": lambda: sp.commit(fd)})
            assert (sx.commit(f) == sx.commit(fd)).all()
        return row(a.label, f"commit_ntt kappa={kappa} n=2^20", ring, f.nbytes / 1e6, measure(calls, a.reps, a.warmup))
    finally:
        xb.close()
        plain.close()


def witness_shapes(a, name):
    wl = make_workload(name)
    ring = wl.ring
    xb, plain = ext_context(ring), api.Context(0, ring=ring)
    out = []
    try:
        L = api._lib()
        for c in (xb, plain):
            c.load_ccs(wl)
        w_ccs = np.ascontiguousarray(wl.w_ccs)
        wd = dev(w_ccs)
        torch.cuda.synchronize()
        if "from_w_ccs" in a.only:
            calls = {"xb_host_ptr": lambda: api.Witness.from_w_ccs(xb, w_ccs).free(), "default_host_ptr": lambda: api.Witness.from_w_ccs(plain, w_ccs).free()}
            if a.dev:
                calls.update({"xb_dev": lambda: api.Witness.from_w_ccs(xb, wd).free(), "default_dev": lambda: api.Witness.from_w_ccs(plain, wd).free()})
            out.append(row(a.label, f"Witness::from_w_ccs {name}", ring, w_ccs.nbytes / 1e6, measure(calls, a.reps, a.warmup)))
        if "get_f" in a.only:
            wx, wp = api.Witness.from_w_ccs(xb, w_ccs), api.Witness.from_w_ccs(plain, w_ccs)
            ho = np.zeros((wl.N, xb.RE), dtype=np.uint64)        # (touched once: no first-touch page faults inside the timed calls)
            do = torch.zeros((wl.N, xb.RE), dtype=torch.int64, device="cuda")
            hp = ho.ctypes.data_as(api.u64p)

            def host_get(c, w):
                rc = L.lf_witness_get_f(c.h, w.h, hp)
                assert rc == 0, rc

            calls = {"xb_host_ptr": lambda: host_get(xb, wx), "default_host_ptr": lambda: host_get(plain, wp)}
            if a.dev:
                calls.update({"xb_dev": lambda: wx.f_into(do), "default_dev": lambda: wp.f_into(do)})
                host_get(xb, wx)
                assert (wx.f_into(do).cpu().numpy().view(np.uint64) == ho).all()
            out.append(row(a.label, f"lf_witness_get_f {name}", ring, ho.nbytes / 1e6, measure(calls, a.reps, a.warmup)))
            wx.free()
            wp.free()
    finally:
        xb.close()
        plain.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ext_basis_io_times.jsonl"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-dev", dest="dev", action="store_false")
    ap.add_argument("--only", nargs="*", default=["commit_gold", "commit_bb", "from_w_ccs", "get_f", "gold", "bb"])
    a = ap.parse_args()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    if "commit_gold" in a.only:
        emit(commit_ntt(a, "goldilocks", 20))
    if "commit_bb" in a.only:
        emit(commit_ntt(a, "babybear", 15))
    if {"from_w_ccs", "get_f"} & set(a.only):
        for ring, name in (("gold", "C4"), ("bb", "C3")):
            if ring in a.only:
                for r in witness_shapes(a, name):
                    emit(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
