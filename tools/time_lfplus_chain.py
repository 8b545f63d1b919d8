"""(GPU box) A LatticeFold+ chain of S proves with its instances built in both forms, alternating step by step in one process:
    python tools/time_lfplus_chain.py [workloads = P16,P17,P20] [steps = 4]
  host   : ComR1CS.new per fresh instance (numpy gadget_decompose, lfplus_commit: host scan + upload of f) + PlusProver.preload (a second upload of f),
  device : PlusProver.ingest (lfplus_witness_from_z: only z crosses PCIe, digits cut and committed in one pass over A).
Step 0 folds L fresh instances, every later step max(1, L - 2) more into the device-resident accumulator (device_acc).  Two provers over the same matrices run
the same chain, one per form; after every step their proofs, accumulators and transcripts are compared word for word BEFORE a time is kept.  Prints one JSON
line per workload: per form the ingestion ms per instance (min / median over the chain's instances), the prove ms and the ms per chained step (min / median
over steps >= 1; step 0 pays the allocations and is reported on its own), and for the kernel `k_ingest` + `k_reduce` the HIP-event ms with the bytes it must
move (A + z read, f written) over that time as a fraction of the 8 TB/s HBM peak."""
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


def flat(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [v for y in x for v in flat(y)]
    return [np.asarray(x)]


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


stat = lambda xs: {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3)} if xs else None
for name in names:
    wl = plus.make_plus_workload(name)
    A, r1cs = wl.ajtai_matrix(), wl.r1cs()
    ncomp = max(1, wl.L - 2)
    provers = {}
    for form in ("host", "device"):
        provers[form] = plus.PlusProver.init(A, list(r1cs), ncomp, wl.params(), plus.PoseidonTranscript(), 0)
        provers[form].device_acc = True
    rec = {form: {"ingest": [], "prove": [], "step": []} for form in provers}
    try:
        nz = 0
        for step in range(steps):
            cnt = wl.L if step == 0 else ncomp
            zs = [wl.z(nz + i) for i in range(cnt)]
            nz += cnt
            out = {}
            for form in (("host", "device") if step % 2 == 0 else ("device", "host")):      # (neither form always runs on the state the other left)
                pr = provers[form]
                t0 = time.perf_counter()
                if form == "host":
                    comps = [plus.ComR1CS.new(pr.ctxs[0], r1cs, z, 1, wl.B, wl.k) for z in zs]
                    pr.preload(comps)
                else:
                    comps = pr.ingest(zs, r1cs)
                t_in = ms_since(t0)
                t1 = time.perf_counter()
                proof = pr.prove(comps)
                t_pr = ms_since(t1)
                out[form] = (proof, [ci.cm_f for ci in comps], t_in, t_pr)
            a, b = flat(out["host"][:2]), flat(out["device"][:2])
            assert len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b)), f"{name} step {step}: the two forms disagree"
            for form, (_, _, t_in, t_pr) in out.items():
                rec[form]["ingest"] += [t_in / cnt] if step else []
                rec[form]["prove"] += [t_pr] if step else []
                rec[form]["step"] += [t_in + t_pr] if step else []
                rec[form].setdefault("step0", {"ingest_per_instance": round(t_in / cnt, 3), "prove": round(t_pr, 3)})
        acc = {form: pr.accumulator() for form, pr in provers.items()}
        assert all((x == y).all() for x, y in zip(acc["host"], acc["device"])), f"{name}: accumulators differ"
        assert provers["host"].transcript.get_challenge() == provers["device"].transcript.get_challenge(), f"{name}: transcripts differ"
        # the kernel alone: HIP events around `iters` passes, z resident, in a context of its own over the same matrix
        kctx = plus.PlusContext(0)
        try:
            kctx.share_matrix(provers["device"].ctxs[0])
            k_ms = kctx.time_witness_from_z(wl.z(0), wl.B, wl.k, 20)
        finally:
            kctx.close()
    finally:
        for pr in provers.values():
            pr.close()
        plus.scratch_trim(0)
    nbytes = (wl.kappa * wl.n + wl.n // wl.k + wl.n) * 128
    res = {"workload": name, "n": wl.n, "L": wl.L, "k": wl.k, "kappa": wl.kappa, "B": wl.B, "steps": steps, "fresh_per_step": ncomp}
    for form in rec:
        res[form] = {"ingest_ms_per_instance": stat(rec[form]["ingest"]), "prove_ms": stat(rec[form]["prove"]), "step_ms": stat(rec[form]["step"]),
                     "step0": rec[form]["step0"]}
    if rec["host"]["ingest"]:
        res["ingest_speedup"] = round(min(rec["host"]["ingest"]) / min(rec["device"]["ingest"]), 2)
    res["kernel"] = {"ms": round(k_ms, 4), "bytes": nbytes, "tb_per_s": round(nbytes / (k_ms * 1e-3) / 1e12, 3), "hbm_frac": round(nbytes / (k_ms * 1e-3) / 8e12, 4)}
    print(json.dumps(res), flush=True)
