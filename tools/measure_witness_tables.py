"""Measurements for DESIGN.md 8e (witness tables; output kept as profiles/witness_tables_measure.txt): python tools/measure_witness_tables.py [fhat] [mz] [spmv_t].
Wall-clock of the calls (each returns with its result complete), median of the repetitions after warm-up."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from latticefold_amd import api
from latticefold_amd.workload import diag, make_workload, splitmix_fq


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def timed(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def show(tag, r, nbytes=None):
    med, lo, hi = r
    bw = f"  {nbytes / med / 1e6:8.1f} GB/s" if nbytes else ""
    print(f"{tag:58s} median {med:9.3f} ms  (min {lo:9.3f}, max {hi:9.3f}){bw}", flush=True)


def fhat(name):
    wl = make_workload(name, 0)
    ctx = api.Context(0, ring=wl.ring)
    ctx.load_ccs(wl)
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    E = wl.RE * 8
    one = torch.empty((wl.tau, wl.m, wl.RE), dtype=torch.int64, device="cuda")
    nb = wl.tau * wl.m * E
    show(f"{name} lf_witness_get_fhat_device, 1 witness ({nb / 1e6:.0f} MB)", timed(lambda: api.get_fhat(ctx, [wit], device=one)), nb)
    show(f"{name} plain fill of equal size", timed(lambda: one.fill_(7)), nb)
    if name == "C4":
        parts = wit.decompose(ctx) + wit.decompose(ctx)
        big = torch.empty((len(parts) * wl.tau, wl.m, wl.RE), dtype=torch.int64, device="cuda")
        nb = len(parts) * wl.tau * wl.m * E
        show(f"{name} lf_witness_get_fhat_device, {len(parts)} witnesses ({nb / 1e9:.1f} GB)", timed(lambda: api.get_fhat(ctx, parts, device=big), reps=5, warm=1), nb)
        show(f"{name} plain fill of equal size", timed(lambda: big.fill_(7), reps=5, warm=1), nb)
        del big, parts
    ctx.close()
    torch.cuda.empty_cache()


def mz(ccs):
    wl = make_workload("C4", 0, ccs=ccs)
    ctx = api.Context(0)
    ctx.load_ccs(wl)
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    out = torch.empty((wl.t, wl.m, wl.RE), dtype=torch.int64, device="cuda")
    head = np.concatenate([wl.x_ccs, diag(1)[None]])
    zbuf = torch.empty((wl.n, wl.RE), dtype=torch.int64, device="cuda")
    wbuf = torch.empty((wl.wit_len, wl.RE), dtype=torch.int64, device="cuda")

    def new():
        wit.mz(wl.x_ccs, device=out)

    def old():   # the parent's only way: w_ccs to the device, z assembled through a device copy, t x lf_spmv_dev
        wit.w_ccs_into(wbuf)
        zbuf[:wl.l + 1] = dev(head)
        zbuf[wl.l + 1:] = wbuf
        for j in range(wl.t):
            ctx.mat_vec_mul(j, zbuf, out=out[j])

    new(); a = out.clone(); old()
    assert torch.equal(a, out)
    for i in range(5):   # interleaved, five runs each
        show(f"C4/{ccs} lf_witness_mz_device               run {i}", timed(new, reps=5, warm=1))
        show(f"C4/{ccs} get_w_ccs_dev + concat + t x spmv  run {i}", timed(old, reps=5, warm=1))
    ctx.close()
    torch.cuda.empty_cache()


def spmv_t():
    wl = make_workload("C4", 0)
    ctx = api.Context(0)
    ctx.load_ccs(wl)
    v = dev(splitmix_fq(3, 0, wl.m * wl.RE).reshape(wl.m, wl.RE))
    z = dev(wl.z())
    on, om = torch.empty((wl.n, wl.RE), dtype=torch.int64, device="cuda"), torch.empty((wl.m, wl.RE), dtype=torch.int64, device="cuda")
    for j in (0, 2):
        nnz = int(wl.rowptr[j][-1])
        show(f"C4/r1cs M_{j} ({nnz} nnz) lf_spmv_t_device", timed(lambda: ctx.mat_vec_mul_t(j, v, out=on)))
        show(f"C4/r1cs M_{j} ({nnz} nnz) lf_spmv_dev", timed(lambda: ctx.mat_vec_mul(j, z, out=om)))
    ctx.close()
    # a C4-sized matrix whose constant column (index l) holds every row, next to the diagonal of the used rows
    rows = min(wl.n, wl.m)
    cnt = np.ones(wl.m, dtype=np.int64)
    cnt[:rows] += 1
    cnt[wl.l] = 1                                             # (the diagonal entry of row l IS the constant column's)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    col = np.full(int(rp[-1]), wl.l, dtype=np.uint32)
    r = np.arange(rows)
    r = r[r != wl.l]
    col[rp[r] + (r > wl.l)] = r                               # CSR columns ascending within a row
    val = splitmix_fq(5, 0, int(rp[-1]) * wl.RE).reshape(-1, wl.RE)
    wl.rowptr[0], wl.col[0], wl.val[0] = rp, col, val
    res = []
    for heavy_min, tag in ((0, "heavy path on (threshold 64)"), (1 << 30, "heavy path off")):
        ctx = api.Context(0)
        ctx.spmv_t_heavy_min(next=heavy_min)
        ctx.load_ccs(wl)
        show(f"C4 constant column of {wl.m} rows: {tag}", timed(lambda: ctx.mat_vec_mul_t(0, v, out=on), reps=5, warm=1))
        res.append(on.clone())
        ctx.close()
    assert torch.equal(res[0], res[1])
    # the threshold: a matrix of 4096 columns of `c` entries each, heavy path on against off
    small = make_workload("T12", 0)
    for c in (16, 32, 64, 128, 256, 1024):
        ncol = min(small.n, 512)
        ent_r = (np.arange(ncol)[:, None] * 7 + np.arange(c)[None, :]) % small.m
        order = np.lexsort((np.repeat(np.arange(ncol), c), ent_r.reshape(-1)))
        rws, cls = ent_r.reshape(-1)[order], np.repeat(np.arange(ncol), c)[order].astype(np.uint32)
        rp = np.concatenate([[0], np.cumsum(np.bincount(rws, minlength=small.m))]).astype(np.uint32)
        small.rowptr[0], small.col[0], small.val[0] = rp, cls, splitmix_fq(9, 0, len(cls) * small.RE).reshape(-1, small.RE)
        vs = dev(splitmix_fq(4, 0, small.m * small.RE).reshape(small.m, small.RE))
        line = []
        for heavy_min in (1, 1 << 30):
            ctx = api.Context(0)
            ctx.spmv_t_heavy_min(next=heavy_min)
            ctx.load_ccs(small)
            o = torch.empty((small.n, small.RE), dtype=torch.int64, device="cuda")
            line.append(timed(lambda: ctx.mat_vec_mul_t(0, vs, out=o), reps=9, warm=2)[0])
            ctx.close()
        print(f"{ncol} columns of {c:5d} entries: every column heavy {line[0]:8.3f} ms, none {line[1]:8.3f} ms", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["fhat", "mz", "spmv_t"]
    if "fhat" in which:
        fhat("C4"); fhat("C3")
    if "mz" in which:
        mz("r1cs"); mz("multi16")
    if "spmv_t" in which:
        spmv_t()
