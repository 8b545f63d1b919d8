"""(GPU box) AjtaiCommitmentScheme::decompose_and_commit_{ntt,coeff} (commitment_scheme.rs:90-113) against what a caller could do without them, on one vector:
    python tools/time_commit_decompose.py [workload] [reps]          (default C4: count 2^18, B 2^16, L 4, kappa 26)
prints one JSON line -- device ms (HIP events around the whole device side, lf_last_kernel_stats) of
  decompose_and_commit_ntt / decompose_and_commit_coeff  (ICRT + gadget digit pass + int8 contraction with ajtai_i8g_planes_base(B) planes),
  Witness::commit of the same vector from a resident Witness.from_w_ccs handle (5 planes),
  commit_ntt of the already-decomposed vector (10 planes),
and the wall ms of the composed host path ntt_inv -> decompose -> ntt_fwd -> commit_ntt (four PCIe round trips).  The four commitments are checked equal.
Repetitions interleave the variants; min and median are reported."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latticefold_amd import api
from latticefold_amd.workload import make_workload

name = sys.argv[1] if len(sys.argv) > 1 else "C4"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
wl = make_workload(name)
B, L, kappa, count = wl.B, wl.L, wl.kappa, len(wl.w_ccs)
ctx = api.Context(0, ring=wl.ring)
ctx.load_ccs(wl)
sch = api.AjtaiCommitmentScheme(ctx, kappa=kappa, n=wl.N, seed=wl.ajtai_seed())
w = np.ascontiguousarray(wl.w_ccs)
coef = ctx.icrt(w)
wit = api.Witness.from_w_ccs(ctx, w)
f_dec = ctx.crt(ctx.decompose(coef, B, L, 0))


def composed():
    return sch.commit_ntt(ctx.crt(ctx.decompose(ctx.icrt(w), B, L, 0)))


runs = {"dc_ntt": lambda: sch.decompose_and_commit_ntt(w, B, L), "dc_coeff": lambda: sch.decompose_and_commit_coeff(coef, B, L),
        "witness_commit": lambda: wit.commit(sch), "commit_ntt_decomposed": lambda: sch.commit_ntt(f_dec)}
planes = api._lib().lfdbg_i8g_planes_base
planes.argtypes, planes.restype = [api.C.c_int, api.C.c_uint64], api.C.c_uint
ref = wit.commit(sch)
dev = {k: [] for k in runs}
wall = []
for it in range(reps + 1):                       # (the first round warms every shape up and is not reported)
    for k, fn in runs.items():
        got = fn()
        assert (got == ref).all(), k
        if it:
            dev[k].append(ctx.kernel_stats()["ajtai_ms"])
    t0 = time.perf_counter()
    got = composed()
    ms = (time.perf_counter() - t0) * 1e3
    assert (got == ref).all(), "composed"
    if it:
        wall.append(ms)
stat = lambda xs: {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4)}
out = {"workload": name, "ring": wl.ring, "count": count, "B": B, "L": L, "kappa": kappa, "width": wl.N, "reps": reps,
       "planes": planes(api.RING_IDS[wl.ring], B),
       "decompose_and_commit_ntt_ms": stat(dev["dc_ntt"]), "decompose_and_commit_coeff_ms": stat(dev["dc_coeff"]),
       "witness_commit_ms": stat(dev["witness_commit"]), "commit_ntt_decomposed_ms": stat(dev["commit_ntt_decomposed"]),
       "composed_host_path_wall_ms": stat(wall)}
ctx.close()
print(json.dumps(out))
