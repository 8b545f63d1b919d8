"""(GPU box) Ring arithmetic on arrays (lfplus_ring_mul, lfplus_spmv, include/lfplus.h) at 2^20 ring elements, host and device form, all cases in one process:
    python tools/time_lfplus_ring_mul.py [--log2 20] [--reps 7] [--only CASE] [--out rows.jsonl]
prints one JSON line per case -- wall ms (min / median over INTERLEAVED repetitions after a dropped warm-up round; every call ends with its own stream
synchronisation, so the wall time of a device form is launch + kernel + the download of the word flag, and that of a host form adds the uploads and the
download of the result) of
  mul_e1 / mul_e3     lfplus_ring_mul, element-wise, n_terms 1 and 3
  mul_b3              lfplus_ring_mul, broadcast, n_terms 3
  spmv                lfplus_spmv with the first of P20's three resident matrices (the gadget-decomposed identity: constant coefficients, two non-zeros in each
                      of the first n / 2 rows, none below)
bytes = what the device form must move through HBM at least once (every input table read, the result written); frac_peak = bytes / min wall time over the
8 TB/s peak, frac_stream = the same over the 4.3 TB/s the slice's streaming passes reach.  For comparison, in the same run: the oracle's
lfp_ring_mul, one call per element from one thread over 2^16 elements (through ctypes: the call overhead is part of the figure).  --only runs the DEVICE form of
one case `reps` times and nothing else: the shape for a `rocprofv3` run of its own."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from latticefold_amd import plus

CASES = ("mul_e1", "mul_e3", "mul_b3", "spmv")
ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", choices=CASES)
ap.add_argument("--out")
args = ap.parse_args()
D, P = plus.D, plus.P
n = 1 << args.log2


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


stat = lambda xs: {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)}
rng = np.random.default_rng(args.log2)
a = rng.integers(0, P, size=(3, n, D), dtype=np.uint64)
b = rng.integers(0, P, size=(3, n, D), dtype=np.uint64)
coef = rng.integers(0, P, size=(3, D), dtype=np.uint64)
dev = lambda x: torch.from_numpy(x.view(np.int64)).cuda()
ad, bd = dev(a), dev(b)
out_h, out_d = np.zeros((n, D), dtype=np.uint64), torch.empty((n, D), dtype=torch.int64, device="cuda")
y_d = torch.empty((n, D), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
ctx = plus.PlusContext(0)
try:
    nnz = 0
    if args.only in (None, "spmv"):
        k, B = 2, plus.make_plus_workload("P20").B
        m = plus.r1cs_decomposed_square((plus.identity_csr(n // k),), n, B, k)[0]      # (P20's three matrices are this one three times)
        ctx.set_matrices([m, m, m], n=n)
        nnz = int(np.asarray(m[0])[-1])
    runs = {
        "mul_e1": (lambda: ctx.ring_mul(a[0], b[0], out=out_h), lambda: ctx.ring_mul(ad[0], bd[0], out=out_d), 3 * n * 128),
        "mul_e3": (lambda: ctx.ring_mul(a, b, out=out_h), lambda: ctx.ring_mul(ad, bd, out=out_d), 7 * n * 128),
        "mul_b3": (lambda: ctx.ring_mul(a, coef, broadcast=True, out=out_h), lambda: ctx.ring_mul(ad, coef, broadcast=True, out=out_d), 4 * n * 128),
        # x gathered once per non-zero, y written, CSR (rowptr, col, one value word)
        "spmv": (lambda: ctx.spmv(0, a[0], out=out_h), lambda: ctx.spmv(0, ad[0], out=y_d), nnz * 128 + n * 128 + (n + 1) * 4 + nnz * 12),
    }
    if args.only:
        for _ in range(args.reps):
            runs[args.only][1]()
        emit({"only": args.only, "log2": args.log2, "reps": args.reps})
        sys.exit(0)
    # the device form gives the host form's words
    for name, (h, d, _) in runs.items():
        h()
        got = d()
        assert np.array_equal(got.cpu().numpy().view(np.uint64), out_h), name
    ms = {(name, form): [] for name in runs for form in ("host", "device")}
    for it in range(args.reps + 1):                 # (the first round warms every shape up and is not reported)
        for name, (h, d, _) in runs.items():
            for form, fn in (("host", h), ("device", d)):
                t = timed(fn)
                if it:
                    ms[(name, form)].append(t)
    for name, (_, _, nbytes) in runs.items():
        dmin = min(ms[(name, "device")])
        emit({"case": name, "elements": n, "reps": args.reps, "host_ms": stat(ms[(name, "host")]), "device_ms": stat(ms[(name, "device")]), "bytes": nbytes,
              "frac_peak": round(nbytes / (dmin * 1e-3) / 8e12, 4), "frac_stream": round(nbytes / (dmin * 1e-3) / 4.3e12, 4)})
    # the oracle: one lfp_ring_mul call per element, one thread
    import lfp
    no = 1 << 16
    lfp.lib()                                        # (builds the oracle if need be)
    f = C.CDLL(lfp._SO).lfp_ring_mul                 # a handle of its own: raw addresses, the cheapest call ctypes has
    f.argtypes, f.restype = [C.c_void_p] * 3, None
    o = np.zeros((no, D), dtype=np.uint64)
    pa, pb, po = a[0].ctypes.data, b[0].ctypes.data, o.ctypes.data
    t0 = time.perf_counter()
    for off in range(0, no * 128, 128):
        f(pa + off, pb + off, po + off)
    t_oracle = (time.perf_counter() - t0) * 1e3
    ctx.ring_mul(a[0], b[0], out=out_h)
    assert np.array_equal(o, out_h[:no]), "the oracle's words"
    emit({"case": "oracle_lfp_ring_mul_loop", "elements": no, "threads": 1, "ms": round(t_oracle, 1), "note": "one ctypes call per element"})
finally:
    ctx.close()
    plus.scratch_trim(0)
