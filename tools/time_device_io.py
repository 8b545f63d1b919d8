#!/usr/bin/env python3
"""Host-pointer call against its `_dev` twin at the shapes a user runs, in one process: wall-clock time of calls that end in the library's own synchronise.

    python tools/time_device_io.py [--reps 9] [--out profiles/device_io_times.jsonl] [--only NAME ...]

Per shape: both variants are warmed up, then `reps` (>= 9) repetitions with the two variants ALTERNATING, host clock around each call.  The host-pointer
variant reads a pageable numpy array (what a ctypes or Rust caller has) and is the behaviour before the `_dev` entry points existed; the device variant reads a
torch tensor that is already resident.  One JSON line per shape: min and median of both variants in ms, the array's size, the ratio of the medians.

Shapes: commit_ntt at the reference's CommitNTT rows (Goldilocks kappa 20, BabyBear kappa 15, n = 2^20), Witness::from_w_ccs, lf_ccs_check and
lf_witness_get_f at C4."""
import argparse
import ctypes as C
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
from latticefold_amd.workload import make_workload, splitmix_fq  # noqa: E402


def dev(a):
    return torch.from_numpy(a.view(np.int64)).to("cuda")


def measure(host_call, dev_call, reps, warmup=2):
    for _ in range(warmup):
        host_call()
        dev_call()
    th, td = [], []
    for _ in range(reps):
        for call, acc in ((host_call, th), (dev_call, td)):
            t0 = time.perf_counter()
            call()
            acc.append((time.perf_counter() - t0) * 1e3)
    return th, td


def row(name, ring, mbytes, th, td):
    r = {"shape": name, "ring": ring, "array_MB": round(mbytes, 1), "reps": len(th),
         "host_ptr_ms": {"min": round(min(th), 3), "median": round(statistics.median(th), 3)},
         "dev_ms": {"min": round(min(td), 3), "median": round(statistics.median(td), 3)}}
    r["median_ratio_host_over_dev"] = round(r["host_ptr_ms"]["median"] / r["dev_ms"]["median"], 2)
    return r


def commit_ntt(ring, kappa, reps):
    n = 1 << 20
    ctx = api.Context(0, ring=ring)
    try:
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=kappa, n=n, seed=7)
        f = splitmix_fq(11, 0, n * ctx.RE, ring).reshape(n, ctx.RE)
        fd = dev(f)
        torch.cuda.synchronize()
        assert (scheme.commit(f) == scheme.commit(fd)).all()
        th, td = measure(lambda: scheme.commit(f), lambda: scheme.commit(fd), reps)
        return row(f"commit_ntt kappa={kappa} n=2^20", ring, f.nbytes / 1e6, th, td)
    finally:
        ctx.close()


def c4_shapes(reps, only):
    wl = make_workload("C4")
    ctx = api.Context(0)
    out = []
    try:
        ctx.load_ccs(wl)
        L = api._lib()
        w_ccs = np.ascontiguousarray(wl.w_ccs)
        wd = dev(w_ccs)
        z = np.ascontiguousarray(wl.z())
        zd = dev(z)
        torch.cuda.synchronize()
        if "from_w_ccs" in only:
            th, td = measure(lambda: api.Witness.from_w_ccs(ctx, w_ccs).free(), lambda: api.Witness.from_w_ccs(ctx, wd).free(), reps)
            out.append(row("Witness::from_w_ccs C4", "goldilocks", w_ccs.nbytes / 1e6, th, td))
        if "ccs_check" in only:
            th, td = measure(lambda: ctx.check_relation(z), lambda: ctx.check_relation(zd), reps)
            out.append(row("lf_ccs_check C4", "goldilocks", z.nbytes / 1e6, th, td))
        if "get_f" in only:
            wit = api.Witness.from_w_ccs(ctx, wd)
            ho = np.zeros((wl.N, ctx.RE), dtype=np.uint64)        # (touched once: no first-touch page faults inside the timed calls)
            do = torch.zeros((wl.N, ctx.RE), dtype=torch.int64, device="cuda")
            hp = ho.ctypes.data_as(api.u64p)

            def host_get():
                rc = L.lf_witness_get_f(ctx.h, wit.h, hp)
                assert rc == 0, rc

            th, td = measure(host_get, lambda: wit.f_into(do), reps)
            assert (do.cpu().numpy().view(np.uint64) == ho).all()
            out.append(row("lf_witness_get_f C4", "goldilocks", ho.nbytes / 1e6, th, td))
            wit.free()
    finally:
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_io_times.jsonl"))
    ap.add_argument("--only", nargs="*", default=["commit_gold", "commit_bb", "from_w_ccs", "ccs_check", "get_f"])
    a = ap.parse_args()
    assert a.reps >= 9
    rows = []
    if "commit_gold" in a.only:
        rows.append(commit_ntt("goldilocks", 20, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if "commit_bb" in a.only:
        rows.append(commit_ntt("babybear", 15, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if {"from_w_ccs", "ccs_check", "get_f"} & set(a.only):
        for r in c4_shapes(a.reps, a.only):
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
