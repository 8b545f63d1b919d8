"""Times lf_fold_step at the C4 shape (2^20 rows, kappa 26, B 2^16) across constraint-system shapes: r1cs and deg3 (the bench envelope, k_lin_round) against
deg5, deg7 and mix8 (the wide envelope, k_lin_round_wide).

    python tools/time_wide_ccs.py [--reps 7] [--config C4] [--out profiles/wide_ccs_times.jsonl] [kinds...]

One child process per kind (a fresh context, one warm-up step), the repetitions interleaved across the kinds: repetition r of every kind runs before repetition
r + 1 of any.  Per step: wall-clock ms and the library's own phase events (lf_last_phase_ms: `linearization` = z, the t M_j z, the s rounds, v and u).  Reports
min and median ms per step and per linearization phase, and next to them the product count of the comb per pair, sum_i (|S_i| - 1) (d + 2), that the wide round
kernel's time is expected to follow.  No oracle run is involved.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def child(config, kind):
    sys.path.insert(0, ROOT)
    import numpy as np
    from latticefold_amd import api
    from latticefold_amd.workload import make_workload
    wl = make_workload(config, 0, ccs=kind)
    ctx = api.Context(0)
    ctx.load_ccs(wl)
    scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
    acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
    products = sum(int(wl.S_off[i + 1] - wl.S_off[i]) - 1 for i in range(wl.q)) * (wl.d + 2)
    print("ready", flush=True)
    for line in sys.stdin:          # one step per line from the parent: the first is the warm-up
        t0 = time.perf_counter()
        api.NIFSProver.prove(ctx, acc, wit, cccs, wit, api.PoseidonTranscript())
        ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"config": config, "ccs": kind, "t": wl.t, "q": wl.q, "d": wl.d, "ms": ms, "phases": ctx.phase_ms(), "comb_products": products,
                          "lin_split_rounds": ctx.lin_split_rounds()}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config", default="C4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_ccs_times.jsonl"))
    ap.add_argument("kinds", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child(a.config, a.child)
    kinds = a.kinds or ["r1cs", "deg3", "deg5", "deg7", "mix8"]
    procs = {k: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--config", a.config, "--child", k], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
             for k in kinds}
    rows = {k: [] for k in kinds}
    try:
        for k in kinds:
            if procs[k].stdout.readline().strip() != "ready":
                raise SystemExit(f"{k}: set-up failed")
        for rep in range(a.reps + 1):
            for k in kinds:
                procs[k].stdin.write("step\n")
                procs[k].stdin.flush()
                line = procs[k].stdout.readline()
                if not line:
                    raise SystemExit(f"{k}: step failed")
                if rep:
                    rows[k].append(json.loads(line))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for k in kinds:
            for r in rows[k]:
                fh.write(json.dumps(r) + "\n")
    for k in kinds:
        ms = [r["ms"] for r in rows[k]]
        lin = [r["phases"]["linearization"] for r in rows[k]]
        r0 = rows[k][0]
        print(f"{a.config}/{k}: t {r0['t']} q {r0['q']} d {r0['d']}; step min {min(ms):.2f} median {statistics.median(ms):.2f} ms; "
              f"linearization min {min(lin):.2f} median {statistics.median(lin):.2f} ms; comb products per pair {r0['comb_products']}; "
              f"split rounds {r0['lin_split_rounds']}")


if __name__ == "__main__":
    main()
