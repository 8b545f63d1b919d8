#!/usr/bin/env python3
"""Host-pointer call against its `_dev` twin at the shapes a user runs, in one process: wall-clock time of calls that end in the library's own synchronise.

    python tools/time_device_io.py [--reps 9] [--out profiles/device_io_times.jsonl] [--only NAME ...] [--append]

Per shape: both variants are warmed up, then `reps` (>= 9) repetitions with the two variants ALTERNATING, host clock around each call.  The host-pointer
variant reads a pageable numpy array (what a ctypes or Rust caller has) and is the behaviour before the `_dev` entry points existed; the device variant reads a
torch tensor that is already resident.  One JSON line per shape: min and median of both variants in ms, the array's size, the ratio of the medians.

Shapes: commit_ntt at the reference's CommitNTT rows (Goldilocks kappa 20, BabyBear kappa 15, n = 2^20), Witness::from_w_ccs, lf_ccs_check and
lf_witness_get_f at C4; the component calls (`--only components`, or one of their names): at C4 decompose / recompose of w_ccs (B, L), linf_check of f (N
elements), build_eq at nv = s and spmv of matrix 0; at C2 (m = 2^16 rows) t = 3 tables for mle_eval_batch, sumcheck_lin_begin, lincomb and horner_combine, and
the 5 + 2 K tau tables of sumcheck_fold_begin; the LatticeFold+ twins (`--only lfplus`, or one of their names) at P20 (2^20 rows): lfplus_set_witness,
lfplus_witness_from_z, lfplus_commit, lfplus_get_witness, and one chained prover step (ingest of the fresh short witnesses + prove) of NativePlusProver."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from latticefold_amd import api  # noqa: E402
from latticefold_amd.workload import make_workload, splitmix_fq  # noqa: E402


def dev(a):
    return torch.from_numpy(a.view(np.int64)).to("cuda")


def measure(host_call, dev_call, reps, warmup=2):
    for _ in range(warmup):
        host_call()
        dev_call()
    th, td = [], []
    for _ in range(reps):
        for call, acc in ((host_call, th), (dev_call, td)):
            t0 = time.perf_counter()
            call()
            acc.append((time.perf_counter() - t0) * 1e3)
    return th, td


def row(name, ring, mbytes, th, td):
    r = {"shape": name, "ring": ring, "array_MB": round(mbytes, 1), "reps": len(th),
         "host_ptr_ms": {"min": round(min(th), 3), "median": round(statistics.median(th), 3)},
         "dev_ms": {"min": round(min(td), 3), "median": round(statistics.median(td), 3)}}
    r["median_ratio_host_over_dev"] = round(r["host_ptr_ms"]["median"] / r["dev_ms"]["median"], 2)
    return r


def commit_ntt(ring, kappa, reps):
    n = 1 << 20
    ctx = api.Context(0, ring=ring)
    try:
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=kappa, n=n, seed=7)
        f = splitmix_fq(11, 0, n * ctx.RE, ring).reshape(n, ctx.RE)
        fd = dev(f)
        torch.cuda.synchronize()
        assert (scheme.commit(f) == scheme.commit(fd)).all()
        th, td = measure(lambda: scheme.commit(f), lambda: scheme.commit(fd), reps)
        return row(f"commit_ntt kappa={kappa} n=2^20", ring, f.nbytes / 1e6, th, td)
    finally:
        ctx.close()


def c4_shapes(reps, only):
    wl = make_workload("C4")
    ctx = api.Context(0)
    out = []
    try:
        ctx.load_ccs(wl)
        L = api._lib()
        w_ccs = np.ascontiguousarray(wl.w_ccs)
        wd = dev(w_ccs)
        z = np.ascontiguousarray(wl.z())
        zd = dev(z)
        torch.cuda.synchronize()
        if "from_w_ccs" in only:
            th, td = measure(lambda: api.Witness.from_w_ccs(ctx, w_ccs).free(), lambda: api.Witness.from_w_ccs(ctx, wd).free(), reps)
            out.append(row("Witness::from_w_ccs C4", "goldilocks", w_ccs.nbytes / 1e6, th, td))
        if "ccs_check" in only:
            th, td = measure(lambda: ctx.check_relation(z), lambda: ctx.check_relation(zd), reps)
            out.append(row("lf_ccs_check C4", "goldilocks", z.nbytes / 1e6, th, td))
        if "get_f" in only:
            wit = api.Witness.from_w_ccs(ctx, wd)
            ho = np.zeros((wl.N, ctx.RE), dtype=np.uint64)        # (touched once: no first-touch page faults inside the timed calls)
            do = torch.zeros((wl.N, ctx.RE), dtype=torch.int64, device="cuda")
            hp = ho.ctypes.data_as(api.u64p)

            def host_get():
                rc = L.lf_witness_get_f(ctx.h, wit.h, hp)
                assert rc == 0, rc

            th, td = measure(host_get, lambda: wit.f_into(do), reps)
            assert (do.cpu().numpy().view(np.uint64) == ho).all()
            out.append(row("lf_witness_get_f C4", "goldilocks", ho.nbytes / 1e6, th, td))
            wit.free()
    finally:
        ctx.close()
    return out


COMPONENTS = ("decompose", "recompose", "linf_check", "build_eq", "mle_eval_batch", "spmv", "sumcheck_lin_begin", "sumcheck_fold_begin", "lincomb",
              "horner_combine")


def component_shapes(reps, only):
    """the ten component calls, element-wise ones at C4 and table calls at C2; each pair is checked for equal results before it is timed.  The host-pointer side
    is timed as the get_f row above: the C entry point itself, on host buffers that exist and have been written before the first timed call (no allocation and
    no first-touch page faults inside a timed call); the device side writes into a tensor that exists"""
    ring = "goldilocks"
    out = []
    tag = "C4"
    L = api._lib()
    rnd = lambda seed, *shape: np.ascontiguousarray(splitmix_fq(seed, 0, int(np.prod(shape)), ring).reshape(shape))
    host = lambda t: t.cpu().numpy().view(np.uint64)
    u = lambda a: a.ctypes.data_as(api.u64p)
    hbuf = lambda *shape: np.ones(shape, dtype=np.uint64)                                   # (written: every page is there)
    dbuf = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")

    def ok(rc):
        assert rc == 0, rc

    def pair(name, arr, host_call, dev_call, same):
        torch.cuda.synchronize()
        host_call()
        dev_call()
        assert same(), name
        th, td = measure(host_call, dev_call, reps)
        out.append(row(f"{name} {tag}", ring, arr.nbytes / 1e6, th, td))

    wl = make_workload("C4")
    ctx = api.Context(0)
    try:
        ctx.load_ccs(wl)
        h, RE, m, s = ctx.h, ctx.RE, wl.m, wl.s
        if "decompose" in only or "recompose" in only:
            x = np.ascontiguousarray(ctx.icrt(wl.w_ccs))
            cnt = wl.wit_len
            xd, ho, do = dev(x), hbuf(cnt * wl.L, RE), dbuf(cnt * wl.L, RE)
            if "decompose" in only:
                pair("lf_decompose", x, lambda: ok(L.lf_decompose(h, u(x), cnt, wl.B, wl.L, 0, u(ho))), lambda: ctx.decompose(xd, wl.B, wl.L, 0, out=do),
                     lambda: (ho == host(do)).all())
            if "recompose" in only:
                d = np.ascontiguousarray(ctx.decompose(x, wl.B, wl.L, 0))
                dd, ho1, do1 = dev(d), hbuf(cnt, RE), dbuf(cnt, RE)
                pair("lf_recompose", d, lambda: ok(L.lf_recompose(h, u(d), cnt, wl.B, wl.L, u(ho1))), lambda: ctx.recompose(dd, wl.B, wl.L, out=do1),
                     lambda: (ho1 == host(do1)).all() and (ho1 == x).all())
        if "linf_check" in only:
            f = np.ascontiguousarray(ctx.crt(ctx.decompose(ctx.icrt(wl.w_ccs), wl.B, wl.L, 0)))
            fd = dev(f)
            got = {}
            okw, mx = C.c_int(), C.c_uint64()

            def host_linf():
                ok(L.lf_linf_check(h, u(f), wl.N, wl.B, 0, C.byref(okw), C.cast(C.byref(mx), api.u64p)))
                got["h"] = (bool(okw.value), mx.value)

            def dev_linf():
                got["d"] = ctx.linf_check(fd, wl.B)

            pair("lf_linf_check", f, host_linf, dev_linf, lambda: got["h"] == got["d"])
        if "build_eq" in only:
            pt = rnd(21, s, ctx.TAU)
            ho, do = hbuf(1 << s, ctx.TAU), dbuf(1 << s, ctx.TAU)
            pair(f"lf_build_eq nv={s}", ho, lambda: ok(L.lf_build_eq(h, u(pt), s, u(ho))), lambda: ctx.build_eq(pt, out=do), lambda: (ho == host(do)).all())
        if "spmv" in only:
            z = np.ascontiguousarray(wl.z())
            zd, ho, do = dev(z), hbuf(m, RE), dbuf(m, RE)
            pair("lf_spmv", z, lambda: ok(L.lf_spmv(h, 0, u(z), u(ho))), lambda: ctx.mat_vec_mul(0, zd, out=do), lambda: (ho == host(do)).all())
    finally:
        ctx.close()
    if not {"mle_eval_batch", "sumcheck_lin_begin", "lincomb", "horner_combine", "sumcheck_fold_begin"} & set(only):
        return out
    wl = make_workload("C2")
    tag = "C2"
    ctx = api.Context(0)
    try:
        ctx.load_ccs(wl)
        h, RE, m, s = ctx.h, ctx.RE, wl.m, wl.s
        if {"mle_eval_batch", "sumcheck_lin_begin", "lincomb", "horner_combine"} & set(only):
            assert wl.t == 3 and m == 1 << 16
            tabs = rnd(22, 3, m, RE)
            td3 = dev(tabs)
            pt = rnd(23, s, ctx.TAU)
            ho, do = hbuf(m, RE), dbuf(m, RE)
            if "mle_eval_batch" in only:
                ev, got = hbuf(3, RE), {}

                def dev_mle():
                    got["d"] = ctx.evaluate_mles(td3, pt)

                pair("lf_mle_eval_batch t=3", tabs, lambda: ok(L.lf_mle_eval_batch(h, u(tabs), 3, m, u(pt), s, u(ev))), dev_mle, lambda: (ev == got["d"]).all())
            if "sumcheck_lin_begin" in only:
                first = lambda t: api.MLSumcheckLin(ctx, t, pt).prove_round()       # (begin alone has no result to compare: the first message stands for it)
                assert (first(tabs) == first(td3)).all()
                pair("lf_sumcheck_lin_begin t=3", tabs, lambda: ok(L.lf_sumcheck_lin_begin(h, u(tabs), u(pt))), lambda: api.MLSumcheckLin(ctx, td3, pt),
                     lambda: True)
            if "lincomb" in only:
                coef = rnd(24, 3, RE)
                pair("lf_lincomb t=3", tabs, lambda: ok(L.lf_lincomb(h, u(coef), u(tabs), 3, m, u(ho))), lambda: api.lincomb(ctx, coef, td3, out=do),
                     lambda: (ho == host(do)).all())
            if "horner_combine" in only:
                ch = rnd(25, 3, ctx.TAU)
                t4d = td3.reshape(3, 1, m, RE)
                pair("lf_horner_combine t=3", tabs, lambda: ok(L.lf_horner_combine(h, u(tabs), 3, 1, m, u(ch), u(ho))),
                     lambda: api.horner_combine(ctx, t4d, ch, out=do), lambda: (ho == host(do)).all())
        if "sumcheck_fold_begin" in only:
            nt = 5 + 2 * wl.K * ctx.TAU
            ftab = rnd(26, nt, m, RE)
            for k, idx in enumerate((0, 2, 4)):       # the eq tables are slot-constant
                ftab[idx] = np.tile(ctx.build_eq(rnd(27 + k, s, ctx.TAU)), (1, 8))
            mu = rnd(30, 2 * wl.K, ctx.TAU)
            fd = dev(ftab)
            first = lambda t: api.MLSumcheckFold(ctx, t, mu).prove_round()
            assert (first(ftab) == first(fd)).all()
            pair(f"lf_sumcheck_fold_begin {nt} tables", ftab, lambda: ok(L.lf_sumcheck_fold_begin(h, u(ftab), u(mu))), lambda: api.MLSumcheckFold(ctx, fd, mu),
                 lambda: True)
    finally:
        ctx.close()
    return out


LFPLUS = ("lfplus_set_witness", "lfplus_witness_from_z", "lfplus_commit", "lfplus_get_witness", "lfplus_chain_step")


def lfplus_shapes(reps, only):
    """the LatticeFold+ twins at P20; each pair is checked for equal results before it is timed, host buffers exist and have been written before the first timed
    call.  The chain step runs two NativePlusProvers side by side -- one ingests host z, the other device z -- and times ingest + prove of a chained step (step 0,
    which pays the allocations, is outside)"""
    from latticefold_amd import plus
    wl = plus.make_plus_workload("P20")
    n, k, B, kappa, D = wl.n, wl.k, wl.B, wl.kappa, plus.D
    ring, out = "frog", []
    host = lambda t: t.cpu().numpy().view(np.uint64)
    u = lambda a: a.ctypes.data_as(plus.u64p)

    def ok(rc):
        assert rc == 0, rc

    def pair(name, arr, host_call, dev_call, same):
        torch.cuda.synchronize()
        host_call()
        dev_call()
        assert same(), name
        th, td = measure(host_call, dev_call, reps)
        out.append(row(f"{name} P20", ring, arr.nbytes / 1e6, th, td))

    z = wl.z(0)
    if set(LFPLUS[:4]) & set(only):
        ctx = plus.PlusContext(0)
        try:
            L = plus._lib()
            ctx.generate_matrix(wl.ajtai_seed, kappa, n)
            f = plus.gadget_decompose(z, B, k)
            fd, zd = dev(f), dev(z)
            got = {}

            def keep(key, fn):
                def call():
                    got[key] = fn()
                return call
            if "lfplus_set_witness" in only:
                pair("lfplus_set_witness", f, lambda: ctx.set_witness(f), lambda: ctx.set_witness(fd), lambda: True)
            if "lfplus_witness_from_z" in only:
                pair("lfplus_witness_from_z", z, keep("h", lambda: ctx.witness_from_z(z, B, k)), keep("d", lambda: ctx.witness_from_z(zd, B, k)),
                     lambda: (got["h"] == got["d"]).all())
            if "lfplus_commit" in only:
                pair("lfplus_commit", f, keep("h", lambda: ctx.commit(f)), keep("d", lambda: ctx.commit(fd)), lambda: (got["h"] == got["d"]).all())
            if "lfplus_get_witness" in only:
                ctx.set_witness(fd)
                ho, do = np.ones((n, D), dtype=np.uint64), torch.zeros((n, D), dtype=torch.int64, device="cuda")
                pair("lfplus_get_witness", ho, lambda: ok(L.lfplus_get_witness(ctx.h, u(ho), n)), lambda: ctx.get_witness(out=do), lambda: (ho == host(do)).all())
        finally:
            ctx.close()
            plus.scratch_trim(0)
    if "lfplus_chain_step" in only:
        r1cs, params, ncomp = wl.r1cs(), wl.params(), max(1, wl.L - 2)
        provers = [plus.NativePlusProver.init(None, list(r1cs), ncomp, params, plus.PoseidonTranscript(), 0, seed=wl.ajtai_seed) for _ in range(2)]
        try:
            zs0 = [wl.z(i) for i in range(wl.L)]
            zs = [wl.z(wl.L + i) for i in range(ncomp)]
            zds = [dev(x) for x in zs]
            torch.cuda.synchronize()
            flats = []
            for pr, first in zip(provers, (zs0, [dev(x) for x in zs0])):
                pr.ingest(first, r1cs)
                flats.append(pr.prove())
            assert (flats[0] == flats[1]).all(), "step 0: the device-z prover differs from the host-z prover"

            def step(pr, fresh):
                def call():
                    pr.ingest(fresh, r1cs)
                    pr.prove()
                return call
            th, td = measure(step(provers[0], zs), step(provers[1], zds), reps)
            assert provers[0].transcript.get_challenge() == provers[1].transcript.get_challenge(), "the two chains end in different states"
            out.append(row(f"NativePlusProver chained step ({ncomp} fresh z) P20", ring, sum(x.nbytes for x in zs) / 1e6, th, td))
        finally:
            for pr in provers:
                pr.close()
            plus.scratch_trim(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_io_times.jsonl"))
    ap.add_argument("--only", nargs="*", default=["commit_gold", "commit_bb", "from_w_ccs", "ccs_check", "get_f", "components"])
    ap.add_argument("--append", action="store_true", help="add the rows to --out, keeping what it holds")
    a = ap.parse_args()
    assert a.reps >= 9
    if "components" in a.only:
        a.only = [x for x in a.only if x != "components"] + list(COMPONENTS)
    if "lfplus" in a.only:
        a.only = [x for x in a.only if x != "lfplus"] + list(LFPLUS)
    rows = []
    if "commit_gold" in a.only:
        rows.append(commit_ntt("goldilocks", 20, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if "commit_bb" in a.only:
        rows.append(commit_ntt("babybear", 15, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if {"from_w_ccs", "ccs_check", "get_f"} & set(a.only):
        for r in c4_shapes(a.reps, a.only):
            rows.append(r)
            print(json.dumps(r), flush=True)
    if set(COMPONENTS) & set(a.only):
        for r in component_shapes(a.reps, a.only):
            rows.append(r)
            print(json.dumps(r), flush=True)
    if set(LFPLUS) & set(a.only):
        for r in lfplus_shapes(a.reps, a.only):
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
