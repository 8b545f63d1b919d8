"""(GPU box) The LatticeFold+ relation checks (lfplus_r1cs_check, lfplus_linb_check) against the work they replace or are a subset of, on one resident instance
per size, all sizes in one process:
    python tools/time_lfplus_check.py [--sizes P16,P17,P20] [--reps 7] [--only r1cs|linb|decompose] [--no-host]
prints one JSON line per size -- wall ms (min / median over INTERLEAVED repetitions, warm; every call ends with its own stream synchronisation, so the wall time is
launch + device + the one download) of
  r1cs_check          lfplus_r1cs_check: A f, the fused residual of the three resident matrices, absmax
  linb_check          lfplus_linb_check at constant points with the three resident matrices: A f, eq / M^T eq weights, one pass over f
  decompose_resident  lfplus_decompose_resident on the same context and points (the LinB check does a strict subset of its work)
and, at the sizes in --host-sizes (default P16), the host route the checks replace: get_witness + the CSR / ring-product reference of
tests/test_gpu_lfplus_check.py.  bytes = what each check must move through HBM at least once, hbm_frac = bytes / min wall time over
the 8 TB/s peak.  --only runs ONE of the calls `reps` times and nothing else: the shape for a `rocprofv3 --kernel-trace --stats` run of its own, whose kernel
durations are the device-side times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from latticefold_amd import plus

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="P16,P17,P20")
ap.add_argument("--host-sizes", default="P16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", choices=("r1cs", "linb", "decompose"))
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()
D = 16


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


stat = lambda xs: {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)}
for name in args.sizes.split(","):
    wl = plus.make_plus_workload(name)
    n, nvars, r1cs = wl.n, wl.nvars, wl.r1cs()
    ctx, d0, d1 = (plus.PlusContext(0) for _ in range(3))
    try:
        ctx.set_matrix(wl.ajtai_matrix())
        ctx.set_matrices(list(r1cs))
        for c in (d0, d1):
            c.share_matrix(ctx)
        cm = ctx.witness_from_z(wl.z(0), wl.B, wl.k)
        res = plus.RESIDENT(3)
        r = np.zeros((nvars, 2, D), dtype=np.uint64)
        r[:, :, 0] = np.random.default_rng(nvars).integers(0, plus.P, size=(nvars, 2), dtype=np.uint64)
        dec = ctx.decompose(None, None, wl.B, r, res, into=(d0, d1))      # the digits of f are 0 / 1: F0 = f, so (C0, v0) is the LinB instance of f itself
        runs = {"r1cs": lambda: ctx.r1cs_check(cm), "linb": lambda: ctx.linb_check(dec["C0"], r, dec["v0"], res),
                "decompose": lambda: ctx.decompose(None, None, wl.B, r, res, into=(d0, d1))}
        assert ctx.r1cs_check(cm)[:3] == (True, 0, n) and ctx.linb_check(dec["C0"], r, dec["v0"], res)[:2] == (True, 0) and (dec["C0"] == cm).all()
        if args.only:
            for _ in range(args.reps):
                runs[args.only]()
            print(json.dumps({"workload": name, "only": args.only, "reps": args.reps}), flush=True)
            continue
        ms = {k: [] for k in runs}
        for it in range(args.reps + 1):                 # (the first round warms every shape up and is not reported)
            for k, fn in runs.items():
                t = timed(fn)
                if it:
                    ms[k].append(t)
        nnz = sum(int(np.asarray(m[0])[-1]) for m in r1cs)
        f_bytes, a_bytes = n * D * 8, wl.kappa * n * D * 8
        # r1cs: A and f for the commitment, f gathered once per matrix (the non-zeros touch each element once per matrix), CSR (rowptr, col, one value word), f for absmax
        r1cs_bytes = a_bytes + f_bytes + 3 * (n + 1) * 4 + nnz * 12 + nnz * D * 8 + f_bytes
        # linb: A and f for the commitment, 8 weight vectors written and read, CSC (colptr, rowidx, one value word) twice, f once
        linb_bytes = a_bytes + f_bytes + 2 * 8 * n * 8 + 2 * (3 * (n + 1) * 4 + nnz * 12) + f_bytes
        out = {"workload": name, "n": n, "kappa": wl.kappa, "reps": args.reps, "r1cs_check_ms": stat(ms["r1cs"]), "linb_check_ms": stat(ms["linb"]),
               "decompose_resident_ms": stat(ms["decompose"]), "r1cs_check_bytes": r1cs_bytes, "linb_check_bytes": linb_bytes,
               "r1cs_check_hbm_frac": round(r1cs_bytes / (min(ms["r1cs"]) * 1e-3) / 8e12, 4), "linb_check_hbm_frac": round(linb_bytes / (min(ms["linb"]) * 1e-3) / 8e12, 4)}
        if not args.no_host and name in args.host_sizes.split(","):
            import lfp
            from test_gpu_lfplus_check import host_first_bad, centred_abs_max
            t0 = time.perf_counter()
            f = ctx.get_witness()
            t1 = time.perf_counter()
            assert host_first_bad(r1cs, f) == n and (lfp.commit(wl.ajtai_matrix(), f) == cm).all() and centred_abs_max(f) <= 1
            out["host_get_witness_ms"] = round((t1 - t0) * 1e3, 1)
            out["host_r1cs_reference_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
        print(json.dumps(out), flush=True)
    finally:
        for c in (d1, d0, ctx):
            c.close()
        plus.scratch_trim(0)
