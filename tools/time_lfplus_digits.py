"""(GPU box) Gadget maps on arrays (lfplus_balanced_decompose, lfplus_balanced_recompose, lfplus_linf_norm, lfplus_set_matrices_gadget; include/lfplus.h), all
cases in one process:
    python tools/time_lfplus_digits.py [--log2 20] [--k 4] [--reps 7] [--limit 300] [--only CASE] [--out profiles/lfplus_digits_times.jsonl]
prints one JSON line per case:
  dec_b2 / dec_b3     lfplus_balanced_decompose_device of 2^log2 elements into k digits, gadget order; b = 2 takes digit_step's shift path, b = 3 its division path
  dec_b2_planes       the same in plane order
  rec_b2 / rec_b3     lfplus_balanced_recompose_device of those digits (2^log2 output elements)
  linf                lfplus_linf_norm_device of 2^log2 elements
event_ms = HIP events recorded on the caller's stream around the call (min / median over INTERLEAVED repetitions after a dropped warm-up round).  The context's
stream is ordered behind the first event (lfplus_ctx_wait_stream) and the call returns after its own stream synchronisation, so the figure is launch + kernel +
the download of the word flag; wall_ms is the host clock around the same call.  bytes = every input byte read once and every output byte written once
((1 + k) x 128 B per element); frac_stream = bytes / min event time over the 4.3 TB/s the slice's streaming passes reach, frac_peak over the
8 TB/s peak.  division_ms = dec_b3 - dec_b2 (min): what the 64-bit signed divisions of the general-b path cost on top of the same bytes.
  gadget / gadget_host_route   an R1CS of three identity matrices over z, m = 2^log2 / k, n = 2^log2: lfplus_set_matrices_gadget (wall ms of the synchronous call:
                      validation, the upload of the short arrays, the expansion on the device) against today's route in the same process,
                      plus.r1cs_decomposed_square (host arithmetic: every coefficient times b^i with Python integers) followed by lfplus_set_matrices (the
                      upload of k times the data and the host transposition), reported separately.
Every case runs under its own time limit (--limit seconds, SIGALRM): a case that exceeds it ends the process at once, with a non-zero status and nothing started
after it.  --only runs one case `reps` times and nothing else: the shape for a profiler run of its own."""
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

CASES = ("dec_b2", "dec_b3", "dec_b2_planes", "rec_b2", "rec_b3", "linf")
ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=20, choices=range(7, 25))
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--only", choices=CASES)
ap.add_argument("--no-gadget", action="store_true")
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("time_lfplus_digits.py: no GPU (nothing is measured without one)")
D, P = plus.D, plus.P
n, k = 1 << args.log2, args.k


def on_alarm(signum, frame):
    sys.stderr.write("time_lfplus_digits.py: a case ran past its time limit; nothing more is started\n")
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


stat = lambda xs: {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4)}
rng = np.random.default_rng(args.log2)
x_d = torch.from_numpy(rng.integers(0, P, size=(n, D), dtype=np.uint64).view(np.int64)).cuda()
dig = {name: torch.empty((n * k, D), dtype=torch.int64, device="cuda") for name in ("b2", "b3", "b2p")}
back_d = torch.empty((n, D), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
ctx = plus.PlusContext(0)
try:
    el = n * 128
    runs = {
        "dec_b2": (lambda: ctx.balanced_decompose(x_d, 2, k, plus.DIGITS_GADGET, out=dig["b2"]), (1 + k) * el),
        "dec_b3": (lambda: ctx.balanced_decompose(x_d, 3, k, plus.DIGITS_GADGET, out=dig["b3"]), (1 + k) * el),
        "dec_b2_planes": (lambda: ctx.balanced_decompose(x_d, 2, k, plus.DIGITS_PLANES, out=dig["b2p"]), (1 + k) * el),
        "rec_b2": (lambda: ctx.balanced_recompose(dig["b2"], 2, k, plus.DIGITS_GADGET, out=back_d), (1 + k) * el),
        "rec_b3": (lambda: ctx.balanced_recompose(dig["b3"], 3, k, plus.DIGITS_GADGET, out=back_d), (1 + k) * el),
        "linf": (lambda: ctx.linf_norm(x_d), el),
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
    # the calls agree with each other on these inputs: the planes are the gadget order transposed
    assert torch.equal(dig["b2"].view(n, k, D).transpose(0, 1).reshape(n * k, D), dig["b2p"]), "plane order differs from gadget order"
    for name, (_, nbytes) in runs.items():
        emin = min(ms[name][0])
        rate = nbytes / (emin * 1e-3)
        emit({"case": name, "elements": n, "k": k, "reps": args.reps, "event_ms": stat(ms[name][0]), "wall_ms": stat(ms[name][1]), "bytes": nbytes,
              "bytes_per_s": round(rate, 0), "frac_stream": round(rate / 4.3e12, 4), "frac_peak": round(rate / 8e12, 4)})
    emit({"case": "division", "elements": n, "k": k, "division_ms": round(min(ms["dec_b3"][0]) - min(ms["dec_b2"][0]), 4),
          "note": "dec_b3 - dec_b2 (min event ms): k 64-bit signed divisions per word on top of the same bytes"})
    if not args.no_gadget:
        m, b = n // k, 2
        short = [plus.identity_csr(m) for _ in range(3)]
        xs = rng.integers(0, P, size=(n, D), dtype=np.uint64)
        new, arith, upload = [], [], []
        for it in range(4):
            signal.alarm(args.limit)
            t0 = time.perf_counter()
            ctx.set_matrices_gadget(short, m, b, k)
            t1 = time.perf_counter()
            signal.alarm(0)
            if it:
                new.append((t1 - t0) * 1e3)
        y_new = ctx.spmv(1, xs)
        for it in range(2):
            signal.alarm(args.limit)
            t0 = time.perf_counter()
            square = plus.r1cs_decomposed_square(short, n, b, k)
            t1 = time.perf_counter()
            ctx.set_matrices(square, n=n)
            t2 = time.perf_counter()
            signal.alarm(0)
            arith.append((t1 - t0) * 1e3)
            upload.append((t2 - t1) * 1e3)
        assert np.array_equal(ctx.spmv(1, xs), y_new), "the gadget-loaded matrices differ from the host-built ones"
        nnz = 3 * m
        emit({"case": "gadget", "n": n, "m": m, "k": k, "b": b, "matrices": 3, "wall_ms": stat(new), "bytes_uploaded": nnz * 132 + 3 * 2 * (m + 1) * 4})
        emit({"case": "gadget_host_route", "n": n, "m": m, "k": k, "b": b, "matrices": 3, "host_arithmetic_ms": stat(arith), "set_matrices_ms": stat(upload),
              "bytes_uploaded": nnz * k * 2 * 132 + 3 * 2 * (n + 1) * 4,
              "note": "plus.r1cs_decomposed_square (Python integers), then lfplus_set_matrices (host transposition, both orientations uploaded)"})
finally:
    ctx.close()
    plus.scratch_trim(0)
