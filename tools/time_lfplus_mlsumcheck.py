#!/usr/bin/env python3
"""Times the generic LatticeFold+ sumcheck (lfplus_mlsumcheck_*) on the R1CS shape -- tables (eq, g_A, g_B, g_C), terms +[0, 1, 2] - [0, 3], degree 3 -- next to
the sumcheck rounds of lfplus_r1cs_linearize in the same process (DESIGN.md section 11 "generic sumcheck").

    python tools/time_lfplus_mlsumcheck.py [--log-n 20] [--reps 5]

Both sides are WALL CLOCK per round, launch to the end of the round's stream synchronisation: the generic rounds around MLSumcheck.prove_round on device tables
(the begin is not timed), the specialised ones as LFPLUS_TIMELINE reports them ("gpu+sync" of every r1cs round, read back from the library's stderr).  The
table words are random: no kernel on either side depends on the values.  Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

os.environ["LFPLUS_TIMELINE"] = "1"            # (read when the library is loaded)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from latticefold_amd import plus  # noqa: E402

D = plus.D


def linearize_rounds(ctx, r1cs, f):
    """us per round of one lfplus_r1cs_linearize, from the library's timeline"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            plus.ComR1CS(tuple(r1cs), None, f, None).linearize(ctx, plus.PoseidonTranscript(), resident=True, preloaded=True)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    return [float(x) for x in re.findall(r"r1cs round\s+\d+: gpu\+sync\s+([0-9.]+) us", text)]


def generic_rounds(ctx, tables, nvars):
    sc = plus.MLSumcheck(ctx, tables, plus.VPoly([(1, [0, 1, 2]), (plus.P - 1, [0, 3])], 3))
    out = []
    for i in range(nvars):
        t0 = time.perf_counter()
        sc.prove_round(None if i == 0 else 12345 + i)
        out.append((time.perf_counter() - t0) * 1e6)
    sc.end()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    nvars, n = a.log_n, 1 << a.log_n
    rng = np.random.default_rng(1)
    f = rng.integers(0, 1 << 62, size=(n, D), dtype=np.uint64)
    val = np.zeros((n, D), dtype=np.uint64)
    val[:, 0] = 1
    r1cs = [(np.arange(n + 1, dtype=np.uint32), rng.permutation(n).astype(np.uint32), val) for _ in range(3)]
    tables = torch.randint(0, 1 << 62, (4, n, D), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx = plus.PlusContext(0)
    ctx.set_matrix(rng.integers(0, 1 << 62, size=(1, n, D), dtype=np.uint64))
    ctx.set_matrices(r1cs)
    ctx.set_witness(f)
    lin, gen = [], []
    for _ in range(a.reps + 1):                  # (the first repetition pays allocations and first launches: dropped)
        lin.append(linearize_rounds(ctx, r1cs, f))
        gen.append(generic_rounds(ctx, tables, nvars))
    lin, gen = np.array(lin[1:]), np.array(gen[1:])
    lmin, gmin = lin.min(axis=0), gen.min(axis=0)
    print(json.dumps({"log_n": nvars, "reps": a.reps, "linearize_rounds_us": round(float(lmin.sum()), 1), "generic_rounds_us": round(float(gmin.sum()), 1),
                      "ratio": round(float(gmin.sum() / lmin.sum()), 2), "linearize_round1_us": round(float(lmin[0]), 1), "generic_round1_us": round(float(gmin[0]), 1),
                      "linearize_per_round_us": [round(float(x), 1) for x in lmin], "generic_per_round_us": [round(float(x), 1) for x in gmin]}))
    ctx.close()


if __name__ == "__main__":
    main()
