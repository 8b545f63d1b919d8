"""(GPU box) The ring products on device memory against the transforms a caller without them pays for, at one size on both rings:
    python tools/time_ring_mul.py [log2_count] [reps] [n_terms]          (default 2^20 elements, 20 repetitions, one term)
prints one JSON line -- HIP-event ms (min / median over interleaved repetitions, warm) of
  lf_ntt_fwd_dev and lf_ntt_inv_dev (the yardsticks: they exist on a library without the products too, where this script times them alone),
  lf_ring_mul_device in NTT form (relayout in, one pass, relayout out -- the shape of one transform),
  lf_ring_mul_device in coefficient form (two forward transforms, the slot products and one inverse transform in one kernel).
`*_stream_frac`: the bytes the call's three arrays amount to (2 n_terms + 1 tables of count ring elements, read or written once) over the best time, as a fraction
of the 6.2 TB/s read stream of DESIGN.md section 2 -- a whole-call figure: the relayout passes and their scratch traffic are in the time, not in the bytes."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latticefold_amd import api
from latticefold_amd.workload import RINGS, splitmix_fq

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
nt = int(sys.argv[3]) if len(sys.argv) > 3 else 1
count = 1 << lg
have = "lf_ring_mul_device" in api.exported_symbols()
STREAM = 6.2e12


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()            # (a _dev call orders the context behind the current stream and returns after its own stream is synchronised)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


out = {"count": count, "n_terms": nt, "reps": reps, "ring_mul": have}
for ring in ("goldilocks", "babybear"):
    RE = RINGS[ring][1]
    ctx = api.Context(0, ring=ring)
    a = dev(splitmix_fq(11, 0, nt * count * RE, ring).reshape(nt, count, RE))
    b = dev(splitmix_fq(12, 0, nt * count * RE, ring).reshape(nt, count, RE))
    o = torch.empty((count, RE), dtype=torch.int64, device="cuda")
    runs = {"ntt_fwd_dev": lambda: ctx.ntt_fwd(a[0], out=o), "ntt_inv_dev": lambda: ctx.ntt_inv(a[0], out=o)}
    if have:
        runs["ring_mul_ntt"] = lambda: ctx.ring_mul(a, b, form="ntt", out=o)
        runs["ring_mul_coeff"] = lambda: ctx.ring_mul(a, b, form="coeff", out=o)
    ms = {k: [] for k in runs}
    for it in range(reps + 2):                   # (the first two rounds warm every shape up and are not reported)
        for k, fn in runs.items():
            t = timed(fn)
            if it >= 2:
                ms[k].append(t)
    if have:                                     # what was timed is what the transforms give
        want = ctx.ntt_inv(ctx.ring_mul(ctx.ntt_fwd(a), ctx.ntt_fwd(b)))
        assert torch.equal(ctx.ring_mul(a, b, form="coeff"), want)
    ctx.close()
    res = {k: {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max": round(max(v), 4)} for k, v in ms.items()}
    res["ntt_fwd_dev"]["stream_frac"] = round(2 * count * RE * 8 / (min(ms["ntt_fwd_dev"]) * 1e-3) / STREAM, 4)
    if have:
        nbytes = (2 * nt + 1) * count * RE * 8
        for k in ("ring_mul_ntt", "ring_mul_coeff"):
            res[k]["bytes"] = nbytes
            res[k]["stream_frac"] = round(nbytes / (min(ms[k]) * 1e-3) / STREAM, 4)
        res["coeff_over_2fwd_1inv"] = round(min(ms["ring_mul_coeff"]) / (2 * min(ms["ntt_fwd_dev"]) + min(ms["ntt_inv_dev"])), 4)
        res["ntt_over_1fwd"] = round(min(ms["ring_mul_ntt"]) / min(ms["ntt_fwd_dev"]), 4)
    out[ring] = res
    del a, b, o
print(json.dumps(out))
