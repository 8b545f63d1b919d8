"""(GPU box) The relation checks (lf_ccs_check, lf_lcccs_check) against the prover work they are a subset of, on one instance:
    python tools/time_relation_check.py [workload] [reps]          (default C4: m 2^20, n 2^18 + 2, r1cs)
prints one JSON line -- wall ms (min / median over interleaved repetitions, warm) of
  lf_ccs_check on z (the PCIe upload of z included),
  lf_lcccs_check on the output of a fold step with bound B (z from the planes, M_j z, eq(r), u, v, cm, norm),
  lf_linearize of the same CCCS, for scale,
and the numpy host residual of tests/test_relation_check_cpu.py at C2, for contrast.  hbm_frac = the bytes lf_ccs_check must read (z + the CSR values)
over its wall time, as a fraction of the 8 TB/s HBM peak (an upper bound on the time: the upload is in it)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from latticefold_amd import api
from latticefold_amd.workload import make_workload
from test_relation_check_cpu import residual_host

name = sys.argv[1] if len(sys.argv) > 1 else "C4"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
wl = make_workload(name)
ctx = api.Context(0, ring=wl.ring)
ctx.load_ccs(wl)
sch = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
cccs = np.concatenate([wit.commit(sch), wl.x_ccs])
z = np.ascontiguousarray(wl.z())
tr = lambda: api.PoseidonTranscript(ring=wl.ring)
acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr())
lc, w1, _ = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr())


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def lin():
    api.LFLinearizationProver.prove(ctx, cccs, wit, tr())


runs = {"ccs_check": lambda: ctx.check_relation(z), "lcccs_check": lambda: ctx.check_lcccs(lc, w1, bound=wl.B), "linearize": lin}
ms = {k: [] for k in runs}
for it in range(reps + 1):                       # (the first round warms every shape up and is not reported)
    for k, fn in runs.items():
        t = timed(fn)
        if it:
            ms[k].append(t)
assert ctx.check_lcccs(lc, w1, bound=wl.B) == set()
ctx.close()
c2 = make_workload("C2")
t0 = time.perf_counter()
assert not residual_host(c2, c2.z()).any()
host_ms = (time.perf_counter() - t0) * 1e3
stat = lambda xs: {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)}
E = wl.RE * 8
bytes_read = wl.n * E + sum(int(np.asarray(rp)[-1]) for rp in wl.rowptr) * E
out = {"workload": name, "ring": wl.ring, "m": wl.m, "n": wl.n, "t": wl.t, "reps": reps,
       "ccs_check_ms": stat(ms["ccs_check"]), "lcccs_check_ms": stat(ms["lcccs_check"]), "linearize_ms": stat(ms["linearize"]),
       "ccs_check_bytes": bytes_read, "ccs_check_hbm_frac": round(bytes_read / (min(ms["ccs_check"]) * 1e-3) / 8e12, 4),
       "host_residual_C2_ms": round(host_ms, 1)}
print(json.dumps(out))
