"""(GPU box) The generic sumcheck (lf_mlsumcheck_*) against the specialised linearization sumcheck (lf_sumcheck_lin_*) on the linearization shape, and on one
shape the specialised path cannot run:
    python tools/time_mlsumcheck.py [workloads, comma separated] [reps]          (default C2,C4: t 3, d 2 at 2^16 and 2^20 rows; 5 repetitions)
prints one JSON line per workload and one for shape (b) (two terms sharing a table, a square, a cube, a single factor; four tables of 2^20 entries).

Both sumchecks run in the split form on device tables with the SAME fixed challenges (no transcript: its host time is the same on both sides), alternating
specialised, generic, specialised, generic ..., warm; every call ends in a device synchronise (each round downloads its message).  Reported per side, wall ms,
min / median: begin (the relayout of the tables into the context), round 1, all rounds.  No existing kernel or launcher differs from the parent commit, so
the specialised side IS the parent's code; the messages of the two sides are compared before anything is reported.
  bytes_round1 = the table bytes of round 1 read once per term that uses them (the generic kernel's traffic when the degree + 1 points fit one point group:
Goldilocks up to degree 3, BabyBear up to degree 2; it re-reads them once per further group).  round1_stream_frac = bytes_round1 / min round-1 wall time as a
fraction of the 6.2 TB/s read-stream rate of DESIGN.md section 2: a LOWER bound on the kernel's fraction (the wall time holds two launches, the download and
the synchronise).  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (k_mls_round / k_mls_finish / k_fix against
k_lin_round / k_reduce_rows)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latticefold_amd import api
from latticefold_amd.workload import RINGS, make_workload, splitmix_fq

names = (sys.argv[1] if len(sys.argv) > 1 else "C2,C4").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
STREAM_BPS = 6.2e12


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stat(xs):
    return {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)}


def run_split(make, nvars, point):
    """begin + nvars rounds of one sumcheck object -> (begin ms, [round ms], messages)"""
    t_begin, sc = timed(make)
    ms, msgs, r = [], [], None
    for i in range(nvars):
        t, m = timed(lambda: sc.prove_round(r))
        ms.append(t); msgs.append(m)
        r = point[i]
    sc.end()
    return t_begin, ms, np.stack(msgs)


def table_bytes(terms, m, ring):
    p, RE, _ = RINGS[ring]
    return sum(len(ix) for _, ix in terms) * m * RE * (8 if ring == "goldilocks" else 4)


for name in names:
    wl = make_workload(name)
    ring, RE, TAU = wl.ring, wl.RE, RINGS[wl.ring][2]
    ctx = api.Context(0, ring=ring)
    ctx.load_ccs(wl)
    beta = splitmix_fq(0xBE7A, 0, wl.s * TAU, ring).reshape(wl.s, TAU)
    point = splitmix_fq(0xC4A1, 0, wl.s * TAU, ring).reshape(wl.s, TAU)
    tables = torch.empty((wl.t + 1, wl.m, RE), dtype=torch.int64, device="cuda")
    zd = torch.from_numpy(np.ascontiguousarray(wl.z()).view(np.int64)).to("cuda")
    for j in range(wl.t):
        ctx.mat_vec_mul(j, zd, out=tables[j])
    eq = torch.empty((wl.m, TAU), dtype=torch.int64, device="cuda")
    ctx.build_eq(beta, out=eq)
    tables[wl.t] = eq.repeat(1, 8)                      # the eq table as a ring table: its tau words in every slot
    torch.cuda.synchronize()
    c = np.asarray(wl.c, dtype=np.uint64).reshape(wl.q, -1)
    terms = [(c[i], [int(j) for j in wl.S_idx[wl.S_off[i]:wl.S_off[i + 1]]] + [wl.t]) for i in range(wl.q)]
    vp = api.VPoly(terms, wl.d + 1)
    res = {"lin": {"begin": [], "round1": [], "rounds": []}, "generic": {"begin": [], "round1": [], "rounds": []}}
    for it in range(reps + 1):                          # (the first repetition warms every shape up and is not reported)
        out = {}
        for side, make in (("lin", lambda: api.MLSumcheckLin(ctx, tables[:wl.t], beta)), ("generic", lambda: api.MLSumcheck(ctx, tables, vp))):
            out[side] = run_split(make, wl.s, point)
            if it:
                res[side]["begin"].append(out[side][0]); res[side]["round1"].append(out[side][1][0]); res[side]["rounds"].append(sum(out[side][1]))
        assert np.array_equal(out["lin"][2], out["generic"][2]), "the two sumchecks give the same messages"
    ctx.close()
    nbytes = table_bytes(terms, wl.m, ring)
    print(json.dumps({"workload": name, "ring": ring, "rows": wl.m, "t": wl.t, "q": wl.q, "degree": wl.d + 1, "reps": reps,
                      "lin_ms": {k: stat(v) for k, v in res["lin"].items()}, "generic_ms": {k: stat(v) for k, v in res["generic"].items()},
                      "rounds_ratio_generic_over_lin": round(min(res["generic"]["rounds"]) / min(res["lin"]["rounds"]), 3),
                      "round1_ratio_generic_over_lin": round(min(res["generic"]["round1"]) / min(res["lin"]["round1"]), 3),
                      "bytes_round1": nbytes, "round1_stream_frac": round(nbytes / (min(res["generic"]["round1"]) * 1e-3) / STREAM_BPS, 3)}), flush=True)
    del tables, eq, zd
    torch.cuda.empty_cache()

# ---- a shape outside the linearization's: (b) at 2^20 entries, Goldilocks ----------------------------------------------------------------------------------
ring, nvars = "goldilocks", 20
p, RE, TAU = RINGS[ring]
ctx = api.Context(0, ring=ring)
tables = torch.randint(0, 2**62, (4, 1 << nvars, RE), dtype=torch.int64, device="cuda")   # (canonical: below p)
torch.cuda.synchronize()
coef = splitmix_fq(0xB0, 0, 5 * RE, ring).reshape(5, RE)
terms = [(coef[0], [0, 1]), (coef[1], [1, 2]), (coef[2], [3, 3]), (coef[3], [2, 2, 2]), (coef[4], [0])]
vp = api.VPoly(terms, 3)
point = splitmix_fq(0xC4A2, 0, nvars * TAU, ring).reshape(nvars, TAU)
begin, round1, rounds = [], [], []
for it in range(reps + 1):
    tb, ms, _ = run_split(lambda: api.MLSumcheck(ctx, tables, vp), nvars, point)
    if it:
        begin.append(tb); round1.append(ms[0]); rounds.append(sum(ms))
ctx.close()
nbytes = table_bytes(terms, 1 << nvars, ring)
print(json.dumps({"shape": "b", "ring": ring, "rows": 1 << nvars, "tables": 4, "terms": 5, "degree": 3, "reps": reps,
                  "generic_ms": {"begin": stat(begin), "round1": stat(round1), "rounds": stat(rounds)},
                  "bytes_round1": nbytes, "round1_stream_frac": round(nbytes / (min(round1) * 1e-3) / STREAM_BPS, 3)}), flush=True)
