"""(GPU box) The decomposed witnesses on the device against the path a caller had before them, on one witness:
    python tools/time_witness_parts.py [workloads, comma separated] [reps]          (default C4,C4b4: N 2^20, K 16 / 8; 7 repetitions)
prints one JSON line per workload -- wall ms (min / median over repetitions that alternate the calls, warm; every call ends in a device synchronise) of
  lf_witness_decompose                                   the K part handles from a witness handle (k_witness_cut),
  lf_witness_recompose                                   the witness back from its K parts (k_witness_join),
  lf_witness_get_f_coeff -> lf_decompose(layout 1) -> K x lf_witness_from_f_coeff      the same K handles through the host, the only way before.
bytes = 4 (K + 1) RE N, what either kernel must move; stream_frac = bytes / min time as a fraction of the 6.2 TB/s read-stream rate of DESIGN.md section 2 (the
wall time holds the launch, the allocations and the synchronise: an upper bound on the kernel's time)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latticefold_amd import api
from latticefold_amd.workload import make_workload

names = (sys.argv[1] if len(sys.argv) > 1 else "C4,C4b4").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
STREAM_BPS = 6.2e12


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def free(ws):
    for w in ws:
        w.free()


for name in names:
    wl = make_workload(name)
    ctx = api.Context(0, ring=wl.ring)
    ctx.load_ccs(wl)
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)

    def host_path():
        parts = ctx.decompose(wit.f_coeff, wl.b, wl.K, 1).reshape(wl.K, wl.N, wl.RE)
        return [api.Witness.from_f_coeff(ctx, p) for p in parts]

    ms = {"decompose": [], "recompose": [], "host_path": []}
    for it in range(reps + 1):                       # (the first round warms every shape up and is not reported)
        t_dec, parts = timed(lambda: wit.decompose(ctx))
        t_rec, back = timed(lambda: api.Witness.recompose(ctx, parts))
        t_host, hparts = timed(host_path)
        if it == 0:                                  # the three agree before anything is reported
            assert (back.f_coeff == wit.f_coeff).all()
            assert all((a.f_coeff == b.f_coeff).all() for a, b in zip(parts, hparts))
        else:
            ms["decompose"].append(t_dec); ms["recompose"].append(t_rec); ms["host_path"].append(t_host)
        free(parts + hparts + [back])
    ctx.close()
    stat = lambda xs: {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)}
    nbytes = 4 * (wl.K + 1) * wl.RE * wl.N
    print(json.dumps({"workload": name, "ring": wl.ring, "N": wl.N, "K": wl.K, "b": wl.b, "reps": reps, "bytes": nbytes,
                      "decompose_ms": stat(ms["decompose"]), "recompose_ms": stat(ms["recompose"]), "host_path_ms": stat(ms["host_path"]),
                      "decompose_stream_frac": round(nbytes / (min(ms["decompose"]) * 1e-3) / STREAM_BPS, 3),
                      "recompose_stream_frac": round(nbytes / (min(ms["recompose"]) * 1e-3) / STREAM_BPS, 3)}), flush=True)
