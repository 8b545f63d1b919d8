#!/usr/bin/env python3
"""Times whole lfplus_prover_prove calls of the prover object on CCS instances (DESIGN.md section 11 "The prover object") against the unchanged R1CS prover
object, interleaved in one process:

    r1cs, r1cs_again   NativePlusProver over ComR1CS (lfplus_prover_create: the yardstick, twice -- the difference between the two is the run-to-run spread)
    ccs_r1cs           NativePlusProver(shape = CCSShape.r1cs()): the same statement through lfplus_ccs_linearize (the general round kernel)
    deg3               t = 4, S = ({0,1,2},{3}), c = (1, -1)
    gate8              t = 8, q_M a b + q_L a + q_R b + q_O c + q_C with a general and a zero coefficient

    python tools/time_lfplus_ccs_prover.py [--workload P20] [--reps 5] [--variants r1cs,ccs_r1cs,deg3,gate8,r1cs_again] [--out profiles/....jsonl]

One repetition = for every variant, in an order that rotates: a fresh prover (commitment matrix generated on the device from the workload's seed), the
workload's L short witnesses ingested (the inputs are RESIDENT when the clock starts), then the timed lfplus_prover_prove of L = nfresh = wl.L instances.
Wall clock around the call, which ends synchronised.  The first repetition pays allocations and first launches and is dropped; the minimum (and the median) of
the others is reported.  At the R1CS shape the payload words of ccs_r1cs are compared with those of r1cs before a time is kept.  Only the r1cs variants use
nothing this file's commit added, so the same file times the R1CS object of an older tree."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from latticefold_amd import plus  # noqa: E402

D = plus.D


def general_coef(seed):
    return np.random.default_rng(seed).integers(0, 1 << 62, size=D, dtype=np.uint64)


SHAPES = {
    "ccs_r1cs": (3, [[0, 1], [2]], [1, -1]),
    "deg3": (4, [[0, 1, 2], [3]], [1, -1]),
    "gate8": (8, [[3, 0, 1], [4, 0], [5, 1], [6, 2], [7]], [1, -1, 5, general_coef(7), 0]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="P20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variants", default="r1cs,ccs_r1cs,deg3,gate8,r1cs_again")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="free text kept in the record (which build this is)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_lfplus_ccs_prover.py: no GPU (nothing is measured without one)")
    wl = plus.make_plus_workload(a.workload)
    r1cs, params = wl.r1cs(), wl.params()
    zs = [wl.z(i) for i in range(wl.L)]
    variants = a.variants.split(",")
    times, flats = {v: [] for v in variants}, {}

    def one(v):
        if v.startswith("r1cs"):
            pr = plus.NativePlusProver.init(None, list(r1cs), 1, params, plus.PoseidonTranscript(), 0, seed=wl.ajtai_seed)
        else:
            sh = SHAPES[v]
            pr = plus.NativePlusProver.init(None, [r1cs[0]] * sh[0], 1, params, plus.PoseidonTranscript(), 0, seed=wl.ajtai_seed, shape=plus.CCSShape(*sh))
        try:
            pr.ingest(zs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flat = pr.prove()
            dt = time.perf_counter() - t0
        finally:
            pr.close()
        return dt, flat

    try:
        for rep in range(a.reps + 1):
            k = rep % len(variants)
            for v in variants[k:] + variants[:k]:
                dt, flat = one(v)
                times[v].append(dt * 1e3)
                if v in ("r1cs", "ccs_r1cs"):
                    flats[v] = flat
            if "r1cs" in flats and "ccs_r1cs" in flats:
                assert np.array_equal(flats["r1cs"][plus.PROOF_HEADER:], flats["ccs_r1cs"][plus.PROOF_HEADER_CCS:]), "the CCS object at the R1CS shape writes other words"
    finally:
        plus.scratch_trim(0)
    res = {"workload": a.workload, "n": wl.n, "L": wl.L, "k": wl.k, "kappa": wl.kappa, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    if a.label:
        res["label"] = a.label
    for v in variants:
        kept = times[v][1:]
        res[v] = {"prove_ms_min": round(min(kept), 3), "prove_ms_median": round(float(np.median(kept)), 3), "dropped_first_ms": round(times[v][0], 3)}
        if not v.startswith("r1cs"):
            sh = SHAPES[v]
            res[v].update(t=sh[0], q=len(sh[1]), d=max(len(S) for S in sh[1]))
    if "r1cs" in res:
        for v in variants:
            if v != "r1cs":
                res[v]["over_r1cs"] = round(res[v]["prove_ms_min"] / res["r1cs"]["prove_ms_min"], 4)
                res[v]["minus_r1cs_ms"] = round(res[v]["prove_ms_min"] - res["r1cs"]["prove_ms_min"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
