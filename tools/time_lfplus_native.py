"""(GPU box) The LatticeFold+ prover object of the C ABI against the Python-orchestrated prover, one chain of S proves, alternating in one process:
    python tools/time_lfplus_native.py [workloads = P16,P17,P20] [steps = 4] [out.jsonl]
  python   : plus.PlusProver (device_acc, ingest form): the schedule in Python over the context-level entry points,
  python2  : a second plus.PlusProver running the same chain -- the difference between the two is the run-to-run spread of this script on this box,
  native   : plus.NativePlusProver (lfplus_prover_ingest + lfplus_prover_prove): the same schedule below the ABI.
Step 0 folds L fresh instances, every later step max(1, L - 2) more into the device-resident accumulator.  The three provers take turns within each step (the
order rotates), and the flat proofs are compared word for word BEFORE a time is kept; accumulators and closing challenges are compared at the end.  A step is
ingest + prove, wall clock.  Prints one JSON line per workload (appended to out.jsonl when given): per prover min / median ms per chained step (steps >= 1;
step 0 pays the allocations and is reported on its own), native / python ratios next to the python2 / python spread, and the seeded-matrix kernel k_fill_ajtai
from HIP events against the bytes it writes."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latticefold_amd import plus

names = (sys.argv[1] if len(sys.argv) > 1 else "P16,P17,P20").split(",")
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
out_path = sys.argv[3] if len(sys.argv) > 3 else None
stat = lambda xs: {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)} if xs else None

for name in names:
    wl = plus.make_plus_workload(name)
    A, r1cs, params = wl.ajtai_matrix(), wl.r1cs(), wl.params()
    ncomp = max(1, wl.L - 2)
    provers = {"python": plus.PlusProver.init(A, list(r1cs), ncomp, params, plus.PoseidonTranscript(), 0),
               "python2": plus.PlusProver.init(A, list(r1cs), ncomp, params, plus.PoseidonTranscript(), 0),
               "native": plus.NativePlusProver.init(A, list(r1cs), ncomp, params, plus.PoseidonTranscript(), 0)}
    for key in ("python", "python2"):
        provers[key].device_acc = True
    order = list(provers)
    rec = {key: {"step": [], "prove": []} for key in provers}
    try:
        nz = 0
        for step in range(steps):
            cnt = wl.L if step == 0 else ncomp
            zs = [wl.z(nz + i) for i in range(cnt)]
            nz += cnt
            flats, times = {}, {}
            for key in order[step % 3:] + order[:step % 3]:      # (no prover always runs on the state another left)
                pr = provers[key]
                t0 = time.perf_counter()
                if key == "native":
                    pr.ingest(zs, r1cs)
                    t1 = time.perf_counter()
                    flats[key] = pr.prove()
                    t2 = time.perf_counter()
                else:
                    comps = pr.ingest(zs, r1cs)
                    t1 = time.perf_counter()
                    proof = pr.prove(comps)
                    t2 = time.perf_counter()
                    flats[key] = plus.proof_to_flat(proof, params, wl.n, len(r1cs))      # (outside the timed span)
                times[key] = ((t2 - t0) * 1e3, (t2 - t1) * 1e3)
            for key in ("python2", "native"):
                assert flats[key].shape == flats["python"].shape and (flats[key] == flats["python"]).all(), f"{name} step {step}: {key} differs from python"
            for key, (t_step, t_prove) in times.items():
                if step:
                    rec[key]["step"].append(t_step)
                    rec[key]["prove"].append(t_prove)
                else:
                    rec[key]["step0"] = round(t_step, 3)
        accs = {key: pr.accumulator() for key, pr in provers.items()}
        chal = {key: pr.transcript.get_challenge() for key, pr in provers.items()}
        for key in ("python2", "native"):
            assert all((x == y).all() for x, y in zip(accs["python"], accs[key])) and chal[key] == chal["python"], f"{name}: {key} ends in another state"
    finally:
        for pr in provers.values():
            pr.close()
        plus.scratch_trim(0)
    # k_fill_ajtai alone: HIP events around `iters` fills of the workload's matrix, in a context of its own
    kctx = plus.PlusContext(0)
    try:
        k_ms = kctx.generate_matrix(wl.ajtai_seed, wl.kappa, wl.n, iters=20)
    finally:
        kctx.close()
        plus.scratch_trim(0)
    nbytes = wl.kappa * wl.n * 128
    res = {"workload": name, "n": wl.n, "L": wl.L, "k": wl.k, "kappa": wl.kappa, "steps": steps, "fresh_per_step": ncomp}
    for key in rec:
        res[key] = {"step_ms": stat(rec[key]["step"]), "prove_ms": stat(rec[key]["prove"]), "step0_ms": rec[key].get("step0")}
    if rec["python"]["step"]:
        m = {key: min(rec[key]["step"]) for key in rec}
        md = {key: float(np.median(rec[key]["step"])) for key in rec}
        res["native_over_python"] = {"min": round(m["native"] / m["python"], 4), "median": round(md["native"] / md["python"], 4)}
        res["python2_over_python"] = {"min": round(m["python2"] / m["python"], 4), "median": round(md["python2"] / md["python"], 4)}
    res["k_fill_ajtai"] = {"ms": round(k_ms, 4), "bytes": nbytes, "tb_per_s": round(nbytes / (k_ms * 1e-3) / 1e12, 3), "hbm_frac": round(nbytes / (k_ms * 1e-3) / 8e12, 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as fh:
            fh.write(line + "\n")
