"""Times lf_fold_step at the C4 shape (2^20 rows, kappa 26, B 2^16) for the decomposition bases (b, K) = (2, 16), (4, 8), (16, 4): configs C4, C4b4, C4b16.

    python tools/time_small_base.py [--reps 7] [--out profiles/small_base_times.jsonl] [names...]

One child process per configuration (a fresh context, one warm-up step), the repetitions interleaved across the configurations: repetition r of every
configuration runs before repetition r + 1 of any.  Per step: wall-clock ms and the library's own phase events (lf_last_phase_ms: decomp_crt_commit = part cut +
part commitments, decomp_evals, fold_prepare, fold_sumcheck, fold_finish) and kernel events (lf_last_kernel_stats: the commit launches, the round launches).
Reports min and median per configuration, and for the commit launch the bytes it must move (A once, the part planes once) over its time as a fraction of the
8 TB/s HBM peak.  No oracle run is involved: C4b4 / C4b16 exist for this timing only.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def child(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    from latticefold_amd import api
    from latticefold_amd.workload import make_workload
    wl = make_workload(name, 0)
    ctx = api.Context(0)
    ctx.load_ccs(wl)
    scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
    acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
    print("ready", flush=True)
    for line in sys.stdin:          # one step per line from the parent: the first is the warm-up
        t0 = time.perf_counter()
        api.NIFSProver.prove(ctx, acc, wit, cccs, wit, api.PoseidonTranscript())
        ms = (time.perf_counter() - t0) * 1e3
        ks = ctx.kernel_stats()
        a_bytes = wl.kappa * wl.N * 24 * 8 + (wl.K - 1) * 24 * wl.N          # byte planes of A once + the part planes (b > 2: one byte per digit)
        print(json.dumps({"config": name, "b": wl.b, "K": wl.K, "ms": ms, "phases": ctx.phase_ms(), "kernels": ks,
                          "commit_bytes": a_bytes}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_base_times.jsonl"))
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    names = a.names or ["C4", "C4b4", "C4b16"]
    procs = {n: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", n], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for n in names}
    rows = {n: [] for n in names}
    try:
        for n in names:
            if procs[n].stdout.readline().strip() != "ready":
                raise SystemExit(f"{n}: set-up failed")
        for rep in range(a.reps + 1):
            for n in names:
                procs[n].stdin.write("step\n")
                procs[n].stdin.flush()
                line = procs[n].stdout.readline()
                if not line:
                    raise SystemExit(f"{n}: step failed")
                if rep:
                    rows[n].append(json.loads(line))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait()
    with open(a.out, "w") as fh:
        for n in names:
            for r in rows[n]:
                fh.write(json.dumps(r) + "\n")
    for n in names:
        ms = [r["ms"] for r in rows[n]]
        com = [r["kernels"]["ajtai_ms"] / max(1, r["kernels"]["ajtai_launches"]) for r in rows[n]]
        frac = rows[n][0]["commit_bytes"] / (min(com) * 1e-3) / 8e12 if min(com) > 0 else 0.0
        ph = {k: statistics.median(r["phases"][k] for r in rows[n]) for k in rows[n][0]["phases"]}
        print(f"{n}: step min {min(ms):.2f} median {statistics.median(ms):.2f} ms; commit launch min {min(com):.3f} ms = {frac:.2f} of 8 TB/s; "
              f"rounds {statistics.median(r['kernels']['fold_round_ms'] for r in rows[n]):.2f} ms; phases (median) " +
              ", ".join(f"{k} {v:.2f}" for k, v in ph.items()))


if __name__ == "__main__":
    main()
