#!/usr/bin/env python3
"""Wall clock of a LatticeFold chain step, three ways on the same library:

    A  call      the call-level overlapped chain: lf_witness_from_w_ccs_begin -> lf_witness_job_finish -> lf_witness_commit -> lf_fold_step -> two lf_witness_free
                 per step (the loop of bench.py's chain extra, copied here), witness j + 1 ingested on lane 2 while step j folds
    B  object    the prover object (lf_prover_*, api.NIFSChainProver) with flags 0
    C  inline    the prover object with LF_PROVER_COMMIT_INLINE
                 (when profiles/chain_prover_times.jsonl was recorded, flags 0 committed the fresh witness inside the ingest job on lane 2; that placement
                 measured slower and was removed -- DESIGN.md 8d -- so B and C now time the same code and their difference is run-to-run spread)

    python tools/time_chain_prover.py                    the whole measurement: per workload (C4, C2) the runs A B C C B A, twice, each run a process of its own
                                                         under its own time limit, stopping at the first run that fails; appends one JSON line per run to
                                                         profiles/chain_prover_times.jsonl and prints the table of DESIGN.md section 8 ("The prover object")
    python tools/time_chain_prover.py --run A --workload C4 [--steps 16]      one run: prints its JSON line

Every run: 2 warm-up steps, then `steps` (>= 16) timed steps bracketed by a device synchronise; fresh transcript per step; the witnesses are generated before
the loop.  The object ingests witness j + 1 straight after prove j returns -- the earliest its state machine allows (one pending instance, one thread)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "chain_prover_times.jsonl")
WARM = 2
ORDER = ("A", "B", "C", "C", "B", "A")
LABEL = {"A": "call-level chain", "B": "object, flags 0", "C": "object, COMMIT_INLINE"}
LIMIT_S = {"C4": 240, "C2": 120}      # time limit of one run (a process of its own)


def run_one(kind, name, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from latticefold_amd import api
    from latticefold_amd.workload import chain_w_ccs, make_workload
    wl = make_workload(name)
    ctx = api.Context(0, ring=wl.ring)
    ctx.load_ccs(wl)
    scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
    tr = lambda: api.PoseidonTranscript(ring=wl.ring)
    ws = [np.ascontiguousarray(chain_w_ccs(wl, j)) for j in range(1, WARM + steps + 1)]
    t_start = None
    if kind == "A":
        w_acc = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        acc, _ = api.LFLinearizationProver.prove(ctx, np.concatenate([w_acc.commit(scheme), wl.x_ccs]), w_acc, tr())
        pending = api.Witness.from_w_ccs_begin(ctx, ws[0])
        for j, w in enumerate(ws):
            if j == WARM:
                torch.cuda.synchronize(0)
                t_start = time.perf_counter()
            w_j = pending.result()
            cccs = np.concatenate([w_j.commit(scheme), wl.x_ccs])
            if j + 1 < len(ws):
                pending = api.Witness.from_w_ccs_begin(ctx, ws[j + 1])
            lc, w_next, proof = api.NIFSProver.prove(ctx, acc, w_acc, cccs, w_j, tr())
            w_j.free(); w_acc.free()
            acc, w_acc = lc, w_next
        torch.cuda.synchronize(0)
        elapsed = time.perf_counter() - t_start
        f = w_acc.f
        w_acc.free()
    else:
        pr = api.NIFSChainProver(ctx, 0 if kind == "B" else api.NIFSChainProver.COMMIT_INLINE)
        pr.init(tr(), wl.w_ccs, wl.x_ccs)
        pr.ingest(ws[0], wl.x_ccs)
        for j, w in enumerate(ws):
            if j == WARM:
                torch.cuda.synchronize(0)
                t_start = time.perf_counter()
            cccs, lc, proof = pr.prove(tr())
            if j + 1 < len(ws):
                pr.ingest(ws[j + 1], wl.x_ccs)
        torch.cuda.synchronize(0)
        elapsed = time.perf_counter() - t_start
        f = pr.accumulator()[1]
        pr.close()
    ok, mx = ctx.linf_check(f, wl.B // 2)
    import hashlib
    rec = {"run": kind, "what": LABEL[kind], "workload": name, "steps": steps, "warmup": WARM, "ms_per_step": elapsed / steps * 1e3,
           "last_proof_sha256": hashlib.sha256(np.ascontiguousarray(proof, dtype=np.uint64).tobytes()).hexdigest(), "folded_norm_below_B_half": bool(ok)}
    ctx.close()
    print(json.dumps(rec))


def table(recs):
    lines = ["| workload | run | ms / step (every run, in order) | median |", "|---|---|---|---|"]
    spread = {}
    for name in sorted({r["workload"] for r in recs}, reverse=True):
        for kind in ("A", "B", "C"):
            v = [r["ms_per_step"] for r in recs if r["workload"] == name and r["run"] == kind]
            if v:
                lines.append(f"| {name} | {kind}: {LABEL[kind]} | {', '.join(f'{x:.2f}' for x in v)} | {statistics.median(v):.2f} |")
            if kind == "A" and v:
                spread[name] = max(v) - min(v)
    for name, s in spread.items():
        lines.append(f"spread of the call-level runs at {name}: {s:.2f} ms")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=("A", "B", "C"))
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--workloads", default="C4,C2")
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    if a.steps < 16:
        ap.error("at least 16 timed steps")
    if a.run:
        run_one(a.run, a.workload, a.steps)
        return 0
    recs = []
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for name in a.workloads.split(","):
        for rep in range(a.repeat):
            for kind in ORDER:
                cmd = ["timeout", "-k", "10", str(LIMIT_S.get(name, 240)), sys.executable, os.path.abspath(__file__), "--run", kind, "--workload", name, "--steps", str(a.steps)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:       # a run that failed, faulted or ran into its limit ends the measurement: nothing more is started on the device
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    print(f"run {kind} at {name} ended with status {p.returncode}: stopping", file=sys.stderr)
                    print(table(recs))
                    return p.returncode
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                rec["pass"] = rep
                recs.append(rec)
                with open(OUT, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")
                print(json.dumps(rec), flush=True)
    print(table(recs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
