#!/usr/bin/env python3
"""Times lfplus_ccs_linearize on a resident witness (DESIGN.md section 11 "CCS instances") against two yardsticks, interleaved in one process:

  (i)  the same shape assembled from the calls the library had before: lfplus_spmv_device x t into one device array of tables, eq(r, .) as a table of RING
       elements, lfplus_mlsumcheck_prove_device on [eq, g_0 ..] with eq a factor of every term.  The eq table is built on the host and uploaded OUTSIDE the
       timed window (a caller would have to build it too: the yardstick is flattered); the two proofs are compared word for word.
  (ii) lfplus_r1cs_linearize, at the R1CS shape only: the hard-wired kernel with its three-product P(0), P(1), P(inf) form.

    python tools/time_lfplus_ccs.py [--log-n 20] [--reps 5] [--shapes r1cs,deg3,gate]

Every figure is WALL CLOCK around a call that ends in a stream synchronisation, the minimum over the repetitions after one dropped warm-up repetition.  Prints
one JSON line per shape."""
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

D, P = plus.D, plus.P


def general_coef(seed):
    return np.random.default_rng(seed).integers(0, 1 << 62, size=D, dtype=np.uint64)


SHAPES = {
    "r1cs": (3, [[0, 1], [2]], [1, -1]),
    "deg3": (4, [[0, 1, 2], [3]], [1, -1]),                                                   # the degree-3 CCS of the bench (--ccs deg3), t = 4
    "gate": (8, [[3, 0, 1], [4, 0], [5, 1], [6, 2], [7]], [1, -1, 5, general_coef(7), 0]),    # q_M a b + q_L a + q_R b + q_O c + q_C
}


def products(sh, generic):
    """negacyclic products per pair and point: sum (|S_i| - 1) + one per general coefficient; the generic path has eq in every term and multiplies by every
    coefficient that is not 0 / +-1"""
    n = 0
    for S, c in zip(sh[1], sh[2]):
        is_int = isinstance(c, (int, np.integer))
        if is_int and c % P == 0:
            continue
        general = not is_int or (generic and c % P not in (1, P - 1))
        n += len(S) - 1 + (1 if generic else 0) + (1 if general else 0)
    return n


def eq_ring_table(r, n):
    w = np.array([1], dtype=object)
    for ri in r:
        ri = int(ri)
        w = np.concatenate([w * (1 - ri) % P, w * ri % P])
    out = np.zeros((n, D), dtype=np.uint64)
    out[:, 0] = w.astype(np.uint64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="r1cs,deg3,gate")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_lfplus_ccs.py: no GPU (nothing is measured without one)")
    nvars, n = a.log_n, 1 << a.log_n
    rng = np.random.default_rng(1)
    f = rng.integers(0, 1 << 62, size=(n, D), dtype=np.uint64)
    f_dev = torch.from_numpy(f.view(np.int64)).cuda()
    val = np.zeros((n, D), dtype=np.uint64)
    val[:, 0] = 1
    A = rng.integers(0, 1 << 62, size=(1, n, D), dtype=np.uint64)
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        t, d = sh[0], max(len(S) for S in sh[1])
        mats = [(np.arange(n + 1, dtype=np.uint32), rng.permutation(n).astype(np.uint32), val) for _ in range(t)]
        ctx = plus.PlusContext(0)
        ctx.set_matrix(A)
        ctx.set_matrices(mats)
        ctx.set_witness(f)
        shape = plus.CCSShape(*sh)
        inst = plus.ComCCS(shape, tuple(mats), None, None, ctx)
        vpoly = plus.VPoly([(c, [0] + [1 + j for j in S]) for S, c in zip(sh[1], sh[2])], d + 1)
        tables = torch.zeros((1 + t, n, D), dtype=torch.int64, device="cuda")
        # the eq table of the generic path, for the challenges a fresh transcript gives (every repetition starts from a fresh transcript)
        tr = plus.PoseidonTranscript()
        r = [tr.get_challenge() for _ in range(nvars)]
        tables[0].copy_(torch.from_numpy(eq_ring_table(r, n).view(np.int64)))
        torch.cuda.synchronize()
        new, gen, hard, same = [], [], [], True
        for _ in range(a.reps + 1):                  # (the first repetition pays allocations and first launches: dropped)
            t0 = time.perf_counter()
            linb, proof = inst.linearize(ctx, plus.PoseidonTranscript(), resident=True)
            new.append(time.perf_counter() - t0)
            tr = plus.PoseidonTranscript()
            for _ in range(nvars):
                tr.get_challenge()
            t0 = time.perf_counter()
            for j in range(t):
                ctx.spmv(j, f_dev, out=tables[1 + j])
            msgs, point, fin = plus.mlsumcheck_prove(ctx, tr, tables, vpoly)
            gen.append(time.perf_counter() - t0)
            same = same and np.array_equal(msgs, proof["msgs"]) and np.array_equal(point, proof["r"]) and np.array_equal(fin[1:], proof["evals"][1:])
            if name == "r1cs":
                t0 = time.perf_counter()
                plus.ComR1CS(tuple(mats), None, None, None, 1, ctx).linearize(ctx, plus.PoseidonTranscript(), resident=True)
                hard.append(time.perf_counter() - t0)
        out = {"shape": name, "log_n": nvars, "reps": a.reps, "t": t, "q": len(sh[1]), "d": d, "products_per_pair_point": products(sh, False),
               "generic_products_per_pair_point": products(sh, True), "ccs_linearize_ms": round(min(new[1:]) * 1e3, 3), "generic_assembled_ms": round(min(gen[1:]) * 1e3, 3),
               "generic_over_ccs": round(min(gen[1:]) / min(new[1:]), 2), "same_words": bool(same)}
        if hard:
            out.update(r1cs_linearize_ms=round(min(hard[1:]) * 1e3, 3), ccs_over_r1cs=round(min(new[1:]) / min(hard[1:]), 2))
        print(json.dumps(out), flush=True)
        ctx.close()
        del tables


if __name__ == "__main__":
    main()
