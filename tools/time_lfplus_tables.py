"""(GPU box) MLE tables on arrays (lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t; include/lfplus.h) at 2^20 entries, the
_device forms, all cases in one process:
    python tools/time_lfplus_tables.py [--log2 20] [--reps 7] [--limit 120] [--only CASE] [--out rows.jsonl]
prints one JSON line per case:
  eq                  lfplus_build_eq_device, nv = log2
  eval1 / eval3       lfplus_mle_eval_batch_device, 1 and 3 tables of 2^log2 general ring elements
  fix1 / fix6 / fixall lfplus_mle_fix_variables_device on 3 tables, nfix = 1, 6 (one launch) and log2 (a chain of launches down to one entry)
  spmv_t              lfplus_spmv_t_device with the first of P20's three resident matrices (the gadget-decomposed identity: constant coefficients, two
                      non-zeros in each of the first n / 2 rows, none below)
event_ms = HIP events recorded on the caller's stream around the call (min / median over INTERLEAVED repetitions after a dropped warm-up round).  The context's
stream is ordered behind the first event (lfplus_ctx_wait_stream) and the call returns after its own stream synchronisation, so the figure is launch + kernel(s)
+ the download of the word flag (and of the result, for eval); wall_ms is the host clock around the same call.  bytes = what the call must move through HBM at
least once (every input read once, the result written); bytes_per_s = bytes / min event time; frac_stream = that over the 4.3 TB/s the slice's streaming
passes reach, frac_peak over the 8 TB/s peak.
  eq_host_route       today's route to the eq factor, in the same process: the table built on the host (Python integers into a numpy array, as
                      tools/time_lfplus_ccs.py (i) does) and uploaded, 128 bytes per row; build and upload are reported separately.
Every case runs under its own time limit (--limit seconds, SIGALRM): a case that exceeds it ends the process at once, with a non-zero status and nothing
started after it.  --only runs one case `reps` times and nothing else: the shape for a `rocprofv3` run of its own."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from latticefold_amd import plus

CASES = ("eq", "eval1", "eval3", "fix1", "fix6", "fixall", "spmv_t")
ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=20, choices=range(7, 25))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--limit", type=int, default=120)
ap.add_argument("--only", choices=CASES)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("time_lfplus_tables.py: no GPU (nothing is measured without one)")
D, P = plus.D, plus.P
nv, n = args.log2, 1 << args.log2


def on_alarm(signum, frame):
    sys.stderr.write("time_lfplus_tables.py: a case ran past its time limit; nothing more is started\n")
    os._exit(3)


signal.signal(signal.SIGALRM, on_alarm)


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def timed(fn):
    """(HIP-event ms, wall ms) of one call, under the case's time limit"""
    signal.alarm(args.limit)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    signal.alarm(0)
    return e0.elapsed_time(e1), wall


def eq_ring_table(r):
    w = np.array([1], dtype=object)
    for ri in r:
        ri = int(ri)
        w = np.concatenate([w * (1 - ri) % P, w * ri % P])
    out = np.zeros((w.size, D), dtype=np.uint64)
    out[:, 0] = w.astype(np.uint64)
    return out


stat = lambda xs: {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4)}
rng = np.random.default_rng(args.log2)
r = rng.integers(0, P, size=nv, dtype=np.uint64)
tabs = torch.from_numpy(rng.integers(0, P, size=(3, n, D), dtype=np.uint64).view(np.int64)).cuda()
eq_d = torch.empty((n, D), dtype=torch.int64, device="cuda")
fix_d = torch.empty((3, n // 2, D), dtype=torch.int64, device="cuda")
fix6_d = torch.empty((3, n >> 6, D), dtype=torch.int64, device="cuda")
fixall_d = torch.empty((3, 1, D), dtype=torch.int64, device="cuda")
y_d = torch.empty((n, D), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
ctx = plus.PlusContext(0)
try:
    nnz = 0
    if args.only in (None, "spmv_t"):
        k, B = 2, plus.make_plus_workload("P20").B
        m = plus.r1cs_decomposed_square((plus.identity_csr(n // k),), n, B, k)[0]      # (P20's three matrices are this one three times)
        ctx.set_matrices([m, m, m], n=n)
        nnz = int(np.asarray(m[0])[-1])
    el = n * 128
    runs = {
        "eq": (lambda: ctx.build_eq(r, out=eq_d), el),
        "eval1": (lambda: ctx.mle_eval_batch(tabs[0], r), el),
        "eval3": (lambda: ctx.mle_eval_batch(tabs, r), 3 * el),
        "fix1": (lambda: ctx.mle_fix_variables(tabs, r[:1], out=fix_d), 3 * el + 3 * el // 2),
        "fix6": (lambda: ctx.mle_fix_variables(tabs, r[:6], out=fix6_d), 3 * el + 3 * el // 64),
        "fixall": (lambda: ctx.mle_fix_variables(tabs, r, out=fixall_d), 3 * el + 2 * (3 * el // 64)),
        # v gathered once per non-zero, the transposed values (one ring element per non-zero), out written, the column pointers and row indices
        "spmv_t": (lambda: ctx.spmv_t(0, tabs[0], out=y_d), 2 * nnz * 128 + el + (n + 1) * 4 + nnz * 4),
    }
    if args.only:
        for _ in range(args.reps):
            timed(runs[args.only][0])
        emit({"only": args.only, "log2": args.log2, "reps": args.reps})
        sys.exit(0)
    ms = {name: ([], []) for name in runs}
    for it in range(args.reps + 1):                 # (the first round warms every shape up and is not reported)
        for name, (fn, _) in runs.items():
            ev, wall = timed(fn)
            if it:
                ms[name][0].append(ev)
                ms[name][1].append(wall)
    # the calls agree with each other on these inputs: fixing every variable leaves the evaluation
    ev3 = ctx.mle_eval_batch(tabs, r)
    assert np.array_equal(fixall_d.cpu().numpy().view(np.uint64)[:, 0], ev3), "fixall differs from eval3"
    for name, (_, nbytes) in runs.items():
        emin = min(ms[name][0])
        rate = nbytes / (emin * 1e-3)
        emit({"case": name, "entries": n, "reps": args.reps, "event_ms": stat(ms[name][0]), "wall_ms": stat(ms[name][1]), "bytes": nbytes,
              "bytes_per_s": round(rate, 0), "frac_stream": round(rate / 4.3e12, 4), "frac_peak": round(rate / 8e12, 4)})
    # today's route to the eq factor: built on the host, uploaded
    build, upload = [], []
    for it in range(3):
        signal.alarm(args.limit)
        t0 = time.perf_counter()
        host_eq = eq_ring_table(r)
        t1 = time.perf_counter()
        eq_up = torch.from_numpy(host_eq.view(np.int64)).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        signal.alarm(0)
        build.append((t1 - t0) * 1e3)
        upload.append((t2 - t1) * 1e3)
    assert torch.equal(eq_up, eq_d), "the device table differs from the host-built one"
    emit({"case": "eq_host_route", "entries": n, "build_ms": stat(build), "upload_ms": stat(upload), "bytes_uploaded": el,
          "note": "numpy table of Python integers + one host-to-device copy, as tools/time_lfplus_ccs.py (i)"})
finally:
    ctx.close()
    plus.scratch_trim(0)
