"""MLE tables on arrays on the device (lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t and their _device forms,
include/lfplus.h) against Python integers (tests/lfplus_tables_ref.py) and against the calls the library already has (lfplus_mlsumcheck_*, lfplus_ring_mul,
lfplus_spmv): host and device memory, the refusals in their stated order, and the independence from everything else a context holds.  Bit-exact: no tolerance.

The thresholds of the implementation (latticefold_amd/csrc/lfp_kernels.h), which the shapes below are derived from:
  TAB_LO = 10     k_tab_eval: a workgroup takes chunks of 2^min(nv, 10) entries, 32 entries per pass and four passes per loop iteration -- at nv >= 10
                  every thread loops 8 times per chunk, the grid of a table is min(chunks, LFPLUS_TABLE_BLOCKS / ntables) workgroups
  TAB_FIX = 6     k_tab_fix: one launch fixes at most 6 variables; nfix = 7 is the first chain of two launches, nfix = 13 the first of three
  SPT_HEAVY = 64  k_spmv_t: a column of MORE than 64 entries is summed by the whole workgroup, 16 entries abreast
  SPT_FLUSH = 64  k_spmv_t: a 16-lane group reduces its lazy sum every 64 products: in the heavy path a column of 16 * 64 = 1024 entries fills every group
                  exactly once, one of 1025 makes the first group flush twice"""
import ctypes as C

import numpy as np
import pytest
import torch

import lfp
import lfplus_mlsumcheck_ref as ref
import lfplus_tables_ref as tref
from latticefold_amd import plus
from test_gpu_lfplus_ring_ops import _rg_read, dev_view, host, margins_intact, mixed_rows, spmv_matrices

pytestmark = pytest.mark.gpu
P, D = plus.P, plus.D
E_ARG = plus.E_ARG
SENT = 0x5A5A5A5A5A5A5A5A
u64p = plus.u64p
TAB_LO, TAB_FIX, SPT_HEAVY, SPT_FLUSH = 10, 6, 64, 64


def L():
    return plus._lib()


def err(ctx):
    return L().lfplus_last_error(ctx.h).decode()


def hp(a):
    return a.ctypes.data_as(u64p)


def vp(x):
    return C.c_void_p(x)


@pytest.fixture(scope="module")
def ctx():
    c = plus.PlusContext(0)      # BARE: no matrix, no witness
    yield c
    c.close()


def points(nv, seed):
    """a random point, and four in which 0, 1, p - 1 and random words take turns"""
    rnd = [int(x) for x in ref.rand_ring(seed, (2 * nv,))]
    out = [rnd[:nv]]
    for s in range(4):
        out.append([(0, 1, P - 1, rnd[nv + i])[(i + s) % 4] for i in range(nv)])
    return [np.array(p, dtype=np.uint64) for p in out]


def pysum(rows):
    return (np.asarray(rows).astype(object).sum(axis=0) % P).astype(np.uint64)


# ---- eq -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", range(1, 7))
def test_eq_against_the_product_formula(ctx, nv):
    for r in points(nv, 0x10 + nv):
        want = tref.eq_words(r)
        got = ctx.build_eq(r)
        assert got.shape == (1 << nv, D) and np.array_equal(got[:, 0], want)
        assert not got[:, 1:].any(), "words 1..15 of every entry are 0"
        ov, ow = dev_view(np.full((1 << nv, D), SENT, dtype=np.uint64))
        assert ctx.build_eq(r, out=ov) is ov and np.array_equal(host(ov), got) and margins_intact(ow)


def test_eq_of_several_chunks_and_as_a_sumcheck_factor(ctx):
    """nv = 13: 32 chunks of 256 entries; the device table as the eq factor of lfplus_mlsumcheck_prove_device gives the messages of a host-built one"""
    nv = 13
    r = points(nv, 0x1D)[1]
    eq_host = np.zeros((1 << nv, D), dtype=np.uint64)
    eq_host[:, 0] = tref.eq_words(r)
    tables = np.concatenate([eq_host[None], ref.rand_ring(0x1E, (2, 1 << nv, D))])
    poly = plus.VPoly([(ref.rand_ring(0x1F, (D,)), [0, 1, 2]), (1, [0, 2])])
    want = plus.mlsumcheck_prove(ctx, plus.PoseidonTranscript(), tables, poly)
    tv, tw = dev_view(tables)
    tv[0].fill_(SENT & 0x7FFFFFFFFFFFFFFF)
    assert ctx.build_eq(r, out=tv[0]) is not None
    assert np.array_equal(host(tv[0]), eq_host) and np.array_equal(host(tv[1:]), tables[1:]) and margins_intact(tw)
    got = plus.mlsumcheck_prove(ctx, plus.PoseidonTranscript(), tv, poly)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(ctx.build_eq(r), eq_host)


# ---- eval -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntables", [1, 3, 64])
@pytest.mark.parametrize("nv", [1, 5])
def test_eval_against_python_integers(ctx, nv, ntables):
    full = mixed_rows(0x200 + 8 * nv + ntables, (ntables, 1 << nv))             # rows of 0, 1 and p - 1 among the random ones
    for ln in sorted({1, (1 << nv) - 1, 1 << nv}):
        tables = np.ascontiguousarray(full[:, :ln])
        for r in points(nv, 0x20 + nv)[:3]:
            want = tref.py_eval(tables, ln, r)
            before = tables.copy()
            got = ctx.mle_eval_batch(tables, r)
            assert np.array_equal(got, want), (ln, r)
            assert np.array_equal(tables, before), "inputs are never written"
            tv, tw = dev_view(tables)
            assert np.array_equal(ctx.mle_eval_batch(tv, r), want) and np.array_equal(host(tv), tables) and margins_intact(tw)
            if ln == 1 << nv:                                                   # fixing every variable leaves the evaluation
                assert np.array_equal(ctx.mle_fix_variables(tables, r)[:, 0], want)
                assert np.array_equal(host(ctx.mle_fix_variables(tv, r))[:, 0], want)
    assert np.array_equal(ctx.mle_eval_batch(full[0], r), want[0]), "the 2-d spelling of one table"


@pytest.mark.parametrize("ntables", [1, 3])
def test_eval_is_the_final_of_a_one_term_sumcheck(ctx, ntables):
    nv = 5
    tables = mixed_rows(0x2A + ntables, (ntables, 1 << nv))
    msgs, point, final = plus.mlsumcheck_prove(ctx, plus.PoseidonTranscript(), tables, plus.VPoly([(1, [0])]))
    assert np.array_equal(ctx.mle_eval_batch(tables, point), final)
    assert np.array_equal(ctx.mle_eval_batch(dev_view(tables)[0], point), final)


@pytest.mark.parametrize("cap", [None, 4])
def test_eval_with_a_looping_thread_and_several_workgroups(ctx, monkeypatch, cap):
    """nv = 12 > TAB_LO: 4 chunks of 1024 entries per table, the last one ragged; every thread loops 8 times (32 passes) per chunk.  Default cap: 4 workgroups per table;
    LFPLUS_TABLE_BLOCKS = 4 with two tables: 2 workgroups per table, each strides over two chunks.  Reference: the eq table times the table through
    lfplus_ring_mul (element-wise, the eq factor a constant polynomial), summed in Python integers"""
    if cap:
        monkeypatch.setenv("LFPLUS_TABLE_BLOCKS", str(cap))
    nv, ntables = 12, 2
    ln = (1 << nv) - 5
    assert ln > 3 << TAB_LO
    tables = ref.rand_ring(0x2C, (ntables, ln, D))
    tables[0, 7] = P - 1
    r = points(nv, 0x2D)[0]
    eq = ctx.build_eq(r)[:ln]
    want = np.stack([pysum(ctx.ring_mul(tables[j], eq)) for j in range(ntables)])
    assert np.array_equal(ctx.mle_eval_batch(tables, r), want)
    tv, tw = dev_view(tables)
    assert np.array_equal(ctx.mle_eval_batch(tv, r), want) and margins_intact(tw)


# ---- fix ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_fix_one_variable_against_python_integers(ctx):
    for nv in (1, 2, 6):
        tables = mixed_rows(0x300 + nv, (3, 1 << nv))
        for r in (0, 1, P - 1, int(ref.rand_ring(0x30, (1,))[0])):
            want = (ref.fix(tables.astype(object), r) % P).astype(np.uint64)
            assert np.array_equal(ctx.mle_fix_variables(tables, [r]), want), (nv, r)
            tv, tw = dev_view(tables)
            ov, ow = dev_view(np.full(want.shape, SENT, dtype=np.uint64))
            assert ctx.mle_fix_variables(tv, [r], out=ov) is ov and np.array_equal(host(ov), want)
            assert np.array_equal(host(tv), tables) and margins_intact(tw) and margins_intact(ow)
    one = ctx.mle_fix_variables(tables[0], [r])
    assert one.shape == (32, D) and np.array_equal(one, want[0]), "the 2-d spelling of one table"


def test_fix_k_variables_at_once_is_k_times_one(ctx):
    """nv = 6, every k <= 6: 32, 16, 8, 4, 2 and 1 output entries per table -- from k = 3 on a wave holds fewer output entries than it has lanes"""
    nv = 6
    tables = mixed_rows(0x31, (3, 1 << nv))
    r = points(nv, 0x32)[2]
    step = tables
    tv, tw = dev_view(tables)
    for k in range(1, nv + 1):
        step = ctx.mle_fix_variables(step, r[k - 1:k])
        assert step.shape == (3, 1 << (nv - k), D)
        assert np.array_equal(ctx.mle_fix_variables(tables, r[:k]), step), k
        assert np.array_equal(host(ctx.mle_fix_variables(tv, r[:k])), step), k
    assert np.array_equal(step, tref.py_fix(tables, r)) and margins_intact(tw)


@pytest.mark.parametrize("nv,nfix", [(7, 7), (8, 7), (13, 13)])
def test_fix_through_a_chain_of_launches(ctx, nv, nfix):
    """more than TAB_FIX variables: two launches (6 + 1), three at nfix = 13 (6 + 6 + 1)"""
    assert nfix > TAB_FIX
    tables = ref.rand_ring(0x33 + nv, (2, 1 << nv, D))
    r = points(nv, 0x34 + nv)[0][:nfix]
    got = ctx.mle_fix_variables(tables, r)
    if nv <= 8:
        assert np.array_equal(got, tref.py_fix(tables, r))
    else:                                                                       # all of them fixed: the evaluation, by another kernel
        assert np.array_equal(got[:, 0], ctx.mle_eval_batch(tables, r))
    step = ctx.mle_fix_variables(ctx.mle_fix_variables(tables, r[:TAB_FIX]), r[TAB_FIX:])
    assert np.array_equal(got, step)
    assert np.array_equal(host(ctx.mle_fix_variables(dev_view(tables)[0], r)), got)


# ---- spmv_t ---------------------------------------------------------------------------------------------------------------------------------------------------------
def threshold_matrix():
    """n = 1030 (a last workgroup of 6 columns).  Columns 3 / 4 hold SPT_HEAVY and SPT_HEAVY + 1 entries (the last light column, the first heavy one), columns
    700 / 1029 hold 16 * SPT_FLUSH and 16 * SPT_FLUSH + 1 (every group of the heavy path full once; the first group flushing twice): rows 0 .. count - 1, every
    coefficient word p - 1.  40 more entries with random coefficients elsewhere; every other column is empty"""
    n = 1030
    special = {3: SPT_HEAVY, 4: SPT_HEAVY + 1, 700: 16 * SPT_FLUSH, 1029: 16 * SPT_FLUSH + 1}
    rng = np.random.default_rng(0x41)
    extra = {int(r): int(c) for r, c in zip(rng.integers(0, n, 40), rng.integers(5, 700, 40))}
    rowptr, col, val = [0], [], []
    rnd = ref.rand_ring(0x42, (n, D))
    for r in range(n):
        for c, cnt in special.items():
            if r < cnt:
                col.append(c)
                val.append(np.full(D, P - 1, dtype=np.uint64))
        if r in extra:
            col.append(extra[r])
            val.append(rnd[r])
        rowptr.append(len(col))
    return n, special, (np.array(rowptr, dtype=np.uint32), np.array(col, dtype=np.uint32), np.stack(val))


@pytest.fixture(scope="module")
def mat_ctx():
    n = 64
    mats = spmv_matrices(n)
    c = plus.PlusContext(0)
    c.set_matrices(mats, n=n)
    yield c, mats, n
    c.close()


def test_spmv_t_against_python_integers(mat_ctx):
    c, mats, n = mat_ctx
    v = mixed_rows(0x43, (n,))
    vv, vw = dev_view(v)
    for j, m in enumerate(mats):
        want = tref.py_spmv_t(m, v)
        assert np.array_equal(c.spmv_t(j, v), want), j
        ov, ow = dev_view(np.full((n, D), SENT, dtype=np.uint64))
        assert c.spmv_t(j, vv, out=ov) is ov and np.array_equal(host(ov), want) and margins_intact(ow)
    assert np.array_equal(host(vv), v) and margins_intact(vw)
    empty = np.setdiff1d(np.arange(n), mats[0][1])
    assert empty.size and not want[empty].any(), "columns without an entry"


def test_spmv_t_at_every_threshold():
    n, special, mat = threshold_matrix()
    c = plus.PlusContext(0)
    try:
        c.set_matrices([mat], n=n)
        full = np.full((n, D), P - 1, dtype=np.uint64)
        got = c.spmv_t(0, full)
        for col, cnt in special.items():                                        # cnt products of (p - 1)(p - 1) per term: c + 1 added, 15 - c subtracted
            row = [((k + 1) - (15 - k)) * cnt * (P - 1) * (P - 1) % P for k in range(D)]
            assert np.array_equal(got[col], np.array(row, dtype=object).astype(np.uint64)), (col, cnt)
        assert np.array_equal(got, tref.py_spmv_t(mat, full))
        v = mixed_rows(0x44, (n,))
        want = tref.py_spmv_t(mat, v)
        assert np.array_equal(c.spmv_t(0, v), want)
        assert np.array_equal(host(c.spmv_t(0, dev_view(v)[0])), want)
        assert not want[[0, 1, 2, 701, 1028]].any(), "empty columns"
        # the order of the entries inside a column does not matter: the same matrix with its rows listed backwards
        perm = np.arange(n)[::-1]
        rp, col, val = mat
        cnt = np.diff(rp)[perm]
        idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in perm])
        c.set_matrices([(np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), col[idx], val[idx])], n=n)
        assert np.array_equal(c.spmv_t(0, np.ascontiguousarray(v[perm])), want)
    finally:
        c.close()


def test_spmv_t_is_the_adjoint_of_spmv(mat_ctx):
    """sum_r (M x)[r] v[r] == sum_c x[c] (M^T v)[c]: the products from lfplus_ring_mul, the sums in Python"""
    c, mats, n = mat_ctx
    x, v = ref.rand_ring(0x45, (n, D)), mixed_rows(0x46, (n,))
    for j in range(len(mats)):
        lhs = pysum(c.ring_mul(c.spmv(j, x), v))
        rhs = pysum(c.ring_mul(x, c.spmv_t(j, v)))
        assert np.array_equal(lhs, rhs) and lhs.any(), j


def test_spmv_t_with_shared_and_replaced_matrices(mat_ctx):
    c, mats, n = mat_ctx
    v = ref.rand_ring(0x47, (n, D))
    want = c.spmv_t(0, v)
    sharer = plus.PlusContext(0)
    try:
        sharer.share_matrices(c)
        assert np.array_equal(sharer.spmv_t(0, v), want)
        other = [ref.rand_csr(0x48, n, 2)]
        sharer.set_matrices(other, n=n)                                          # the sharer lets go; the owner keeps its own
        got = sharer.spmv_t(0, v)
        assert np.array_equal(got, tref.py_spmv_t(other[0], v)) and not np.array_equal(got, want)
        assert np.array_equal(c.spmv_t(0, v), want)
    finally:
        sharer.close()


def test_the_four_together(mat_ctx):
    """mle_eval_batch(M_j f)(r) == sum_c f[c] (M_j^T eq(r))[c] at n = 64, in both memory spaces"""
    c, mats, n = mat_ctx
    r = points(6, 0x49)[0]
    f = ref.rand_ring(0x4A, (n, D))
    fv = dev_view(f)[0]
    for j in range(len(mats)):
        lhs = c.mle_eval_batch(c.spmv(j, f), r)
        w = c.spmv_t(j, c.build_eq(r))
        assert np.array_equal(lhs, pysum(c.ring_mul(f, w))) and lhs.any(), j
        eqd = c.build_eq(r, out=dev_view(np.zeros((n, D), dtype=np.uint64))[0])
        wd = c.spmv_t(j, eqd)
        assert np.array_equal(host(wd), w)
        assert np.array_equal(c.mle_eval_batch(c.spmv(j, fv), r), lhs)
        assert np.array_equal(c.mle_fix_variables(c.spmv(j, f), r)[0], lhs)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_stated_order(ctx):
    nv, nt = 3, 2
    ln = 1 << nv
    t = ref.rand_ring(0x51, (nt, ln, D))
    pt = ref.rand_ring(0x52, (nv,))
    badpt = pt.copy()
    badpt[1] = P
    out = np.full((nt * ln, D), SENT, dtype=np.uint64)
    lib = L()
    calls = {     # name -> (host call, device call) of (context, tables, point, out, count arguments)
        "eq": (lambda c, T, p, o, nv_=nv: lib.lfplus_build_eq(c.h, p, nv_, o), lambda c, T, p, o, nv_=nv: lib.lfplus_build_eq_device(c.h, p, nv_, o)),
        "eval": (lambda c, T, p, o, a=(nt, ln, nv): lib.lfplus_mle_eval_batch(c.h, T, a[0], a[1], p, a[2], o),
                 lambda c, T, p, o, a=(nt, ln, nv): lib.lfplus_mle_eval_batch_device(c.h, T, a[0], a[1], p, a[2], o)),
        "fix": (lambda c, T, p, o, a=(nt, ln, 2): lib.lfplus_mle_fix_variables(c.h, T, a[0], a[1], p, a[2], o),
                lambda c, T, p, o, a=(nt, ln, 2): lib.lfplus_mle_fix_variables_device(c.h, T, a[0], a[1], p, a[2], o)),
    }
    bad_counts = {"eq": [0, 29], "eval": [(0, ln, nv), (65, ln, nv), (nt, 0, nv), (nt, ln + 1, nv), (nt, ln, 0), (nt, ln, 29)],
                  "fix": [(0, ln, 2), (65, ln, 2), (nt, ln - 1, 2), (nt, 1, 1), (nt, ln, 0), (nt, ln, nv + 1), (nt, 1 << 29, 2)]}
    sharded = plus.PlusContext(0)
    try:
        sharded.set_sharding_model(0, 2)
        for name, (h, d) in calls.items():
            # a NULL array, before the envelope
            for T, p, o in ((None, hp(pt), hp(out)), (hp(t), None, hp(out)), (hp(t), hp(pt), None)):
                if name == "eq" and T is None:
                    continue
                assert h(ctx, T, p, o, bad_counts[name][0]) == E_ARG and "null" in err(ctx), name
            assert d(ctx, None, None, None, bad_counts[name][0]) == E_ARG and "null" in err(ctx), name
            # the envelope, before the sharded context
            for c in (ctx, sharded):
                for a in bad_counts[name]:
                    assert h(c, hp(t), hp(pt), hp(out), a) == E_ARG and "envelope" in err(c), (name, a)
            # the sharded context, before the overlap rule and the pointer checks
            assert h(sharded, hp(t), hp(pt), hp(pt)) == E_ARG and "sharded" in err(sharded), name
            assert d(sharded, vp(t.ctypes.data), hp(pt), hp(out) if name == "eval" else vp(out.ctypes.data)) == E_ARG and "sharded" in err(sharded), name
            # out overlapping an input, before the point is tested
            assert h(ctx, hp(t), hp(badpt), hp(badpt)) == E_ARG and "overlaps" in err(ctx), name
            if name != "eq":
                assert h(ctx, hp(t), hp(badpt), C.cast(vp(t.ctypes.data + 64), u64p)) == E_ARG and "overlaps" in err(ctx), name
            # ... before the pointer checks: host addresses in the device form
            if name == "eval":
                assert d(ctx, vp(t.ctypes.data), hp(badpt), hp(badpt)) == E_ARG and "overlaps" in err(ctx)
            if name == "fix":
                assert d(ctx, vp(t.ctypes.data), hp(badpt), vp(t.ctypes.data + 128)) == E_ARG and "overlaps" in err(ctx)
            # the pointer checks, before the point is tested
            assert d(ctx, vp(t.ctypes.data), hp(badpt), hp(out) if name == "eval" else vp(out.ctypes.data)) == E_ARG and "device memory" in err(ctx), name
            # a point word >= p, before the tables are looked at
            badt = t.copy()
            badt[1, 2, 3] = P
            assert h(ctx, hp(badt), hp(badpt), hp(out)) == E_ARG and "non-canonical word in point" in err(ctx), name
            if name != "eq":
                assert h(ctx, hp(badt), hp(pt), hp(out)) == E_ARG and "non-canonical word in tables" in err(ctx), name
        assert (out == SENT).all(), "the host out is untouched"
        assert np.array_equal(ctx.mle_eval_batch(t, pt), tref.py_eval(t, ln, pt)), "the context stays usable"
    finally:
        sharded.close()


def test_device_pointer_refusals_and_device_words(ctx):
    nv, nt = 3, 2
    ln = 1 << nv
    t = ref.rand_ring(0x53, (nt, ln, D))
    pt = ref.rand_ring(0x54, (nv,))
    tv, tw = dev_view(t)
    ov, ow = dev_view(np.full((nt * ln, D), SENT, dtype=np.uint64))
    hout = np.full((nt, D), SENT, dtype=np.uint64)
    torch.cuda.empty_cache()
    big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")      # an allocation of its own (requested from an empty cache)
    pinned = torch.zeros((nt * ln, D), dtype=torch.int64).pin_memory()
    pageable = np.zeros((nt * ln, D), dtype=np.uint64)
    torch.cuda.synchronize()
    lib = L()
    for name, addr in (("pinned host memory", lambda good: pinned.data_ptr()), ("pageable host memory", lambda good: pageable.ctypes.data),
                       ("dev + 8", lambda good: good + 8), ("off the end", lambda good: big.data_ptr() + (32 << 20) - 128)):
        assert lib.lfplus_build_eq_device(ctx.h, hp(pt), nv, vp(addr(ov.data_ptr()))) == E_ARG and "device memory" in err(ctx), name
        assert lib.lfplus_mle_eval_batch_device(ctx.h, vp(addr(tv.data_ptr())), nt, ln, hp(pt), nv, hp(hout)) == E_ARG and "device memory" in err(ctx), name
        assert lib.lfplus_mle_fix_variables_device(ctx.h, vp(addr(tv.data_ptr())), nt, ln, hp(pt), 1, vp(ov.data_ptr())) == E_ARG and "device memory" in err(ctx), name
        assert lib.lfplus_mle_fix_variables_device(ctx.h, vp(tv.data_ptr()), nt, ln, hp(pt), 1, vp(addr(ov.data_ptr()))) == E_ARG and "device memory" in err(ctx), name
    assert (host(ov) == SENT).all() and (hout == SENT).all() and np.array_equal(host(tv), t)
    # a device word >= p: found by the kernel that reads it, the host out untouched
    for pos, word in (((0, 0, 0), P), ((nt - 1, ln - 1, D - 1), 2**64 - 1)):
        bad = t.copy()
        bad[pos] = word
        bv, bw = dev_view(bad)
        ctx.wait_stream()
        assert lib.lfplus_mle_eval_batch_device(ctx.h, vp(bv.data_ptr()), nt, ln, hp(pt), nv, hp(hout)) == E_ARG and "non-canonical word in tables" in err(ctx)
        assert lib.lfplus_mle_fix_variables_device(ctx.h, vp(bv.data_ptr()), nt, ln, hp(pt), 2, vp(ov.data_ptr())) == E_ARG and "non-canonical word in tables" in err(ctx)
        assert lib.lfplus_mle_fix_variables(ctx.h, hp(bad), nt, ln, hp(pt), 2, hp(pageable)) == E_ARG and "non-canonical word in tables" in err(ctx)
        assert (hout == SENT).all() and not pageable.any() and margins_intact(ow) and margins_intact(bw)
    # the same arrays, well-formed
    assert lib.lfplus_mle_eval_batch_device(ctx.h, vp(tv.data_ptr()), nt, ln, hp(pt), nv, hp(hout)) == 0 and np.array_equal(hout, tref.py_eval(t, ln, pt))
    assert lib.lfplus_mle_fix_variables_device(ctx.h, vp(tv.data_ptr()), nt, ln, hp(pt), nv, vp(ov.data_ptr())) == 0
    assert np.array_equal(host(ov)[:nt], hout) and margins_intact(tw) and margins_intact(ow)


def test_spmv_t_refusals_in_their_stated_order():
    n = 64
    v, out = mixed_rows(0x55, (n,)), np.full((n, D), SENT, dtype=np.uint64)
    bad = v.copy()
    bad[n - 1, D - 1] = P
    lib = L()
    c, sharded = plus.PlusContext(0), plus.PlusContext(0)
    try:
        sharded.set_sharding_model(0, 2)
        assert lib.lfplus_spmv_t(c.h, 9, None, n + 1, hp(out)) == E_ARG and "null" in err(c)
        assert lib.lfplus_spmv_t_device(c.h, 9, None, n + 1, None) == E_ARG and "null" in err(c)
        for x in (c, sharded):                                                   # the state of the matrices, before the sharded context
            assert lib.lfplus_spmv_t(x.h, 9, hp(v), n + 1, hp(v)) == E_ARG and "no resident matrices" in err(x)
            x.set_matrices(spmv_matrices(n), n=n)
            assert lib.lfplus_spmv_t(x.h, 2, hp(v), n + 1, hp(v)) == E_ARG and "matrix 2 of 2" in err(x)
            assert lib.lfplus_spmv_t(x.h, 1, hp(v), n + 1, hp(v)) == E_ARG and "wide" in err(x)
        assert lib.lfplus_spmv_t(sharded.h, 0, hp(v), n, hp(v)) == E_ARG and "sharded" in err(sharded)
        assert lib.lfplus_spmv_t_device(sharded.h, 0, vp(v.ctypes.data), n, vp(v.ctypes.data)) == E_ARG and "sharded" in err(sharded)
        # overlap before the pointer checks, the pointer checks before the words
        assert lib.lfplus_spmv_t(c.h, 0, hp(bad), n, hp(bad)) == E_ARG and "overlaps" in err(c)
        assert lib.lfplus_spmv_t(c.h, 0, hp(bad), n, C.cast(vp(bad.ctypes.data + (n - 1) * D * 8), u64p)) == E_ARG and "overlaps" in err(c)
        assert lib.lfplus_spmv_t_device(c.h, 0, vp(bad.ctypes.data), n, vp(bad.ctypes.data + 128)) == E_ARG and "overlaps" in err(c)
        bv, bw = dev_view(bad)
        ov, ow = dev_view(out)
        torch.cuda.empty_cache()
        big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        off_end = big.data_ptr() + (32 << 20) - 128
        for pv, po in ((bad.ctypes.data, ov.data_ptr()), (bv.data_ptr() + 8, ov.data_ptr()), (bv.data_ptr(), out.ctypes.data), (bv.data_ptr(), ov.data_ptr() + 8),
                       (bv.data_ptr(), off_end), (off_end, ov.data_ptr())):
            assert lib.lfplus_spmv_t_device(c.h, 0, vp(pv), n, vp(po)) == E_ARG and "device memory" in err(c)
        assert (host(ov) == SENT).all()
        c.wait_stream()
        assert lib.lfplus_spmv_t_device(c.h, 0, vp(bv.data_ptr()), n, vp(ov.data_ptr())) == E_ARG and "non-canonical word in v" in err(c)
        assert lib.lfplus_spmv_t(c.h, 0, hp(bad), n, hp(out)) == E_ARG and "non-canonical word in v" in err(c)
        assert (out == SENT).all() and margins_intact(ow) and margins_intact(bw), "the host out is untouched"
        assert np.array_equal(c.spmv_t(1, v), tref.py_spmv_t(spmv_matrices(n)[1], v)), "the context stays usable"
    finally:
        c.close()
        sharded.close()


# ---- independence ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pending", [False, True])
def test_a_loaded_context_is_not_disturbed(pending):
    """a matrix, a witness, a from_f pass (pending on the second stream or collected) and a generic sumcheck in its second round: the eight calls in between
    change none of the words that come out afterwards"""
    n, kappa, k = 1 << 15, 1, 2                                               # (from_f needs n > kappa k d l d)
    dp = plus.DecompParameters.for_frog(k)
    A = lfp.splitmix(1, 0, kappa * n * D).reshape(kappa, n, D) % np.uint64(P)
    w = (lfp.splitmix(2, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    f = np.where(w < 0, np.uint64(P) - (-w).astype(np.uint64), w.astype(np.uint64)).reshape(n, D)
    r1cs = [ref.rand_csr(0x55 + q, n, 1) for q in range(3)]
    tables, terms, degree, msgs, point, final = ref.case("b", 4)
    small = mixed_rows(0x61, (3, 32))
    r = points(5, 0x62)[1]
    xs = ref.rand_ring(0x63, (n, D))
    c = plus.PlusContext(0)
    try:
        c.set_matrix(A)
        c.set_matrices(r1cs)
        c.set_witness(f)
        c._chk(L().lfplus_rg_from_f(c.h, dp.b, dp.k, dp.l))
        want = _rg_read(c, k, kappa, n)
        c._chk((L().lfplus_rg_from_f_async if pending else L().lfplus_rg_from_f)(c.h, dp.b, dp.k, dp.l))
        sc = plus.MLSumcheck(c, tables, plus.VPoly(terms, degree))
        assert np.array_equal(sc.prove_round(), msgs[0])
        assert np.array_equal(sc.prove_round(int(point[0])), msgs[1])
        # the calls under test, host and device form
        sv = dev_view(small)[0]
        eq = c.build_eq(r)
        assert np.array_equal(eq[:, 0], tref.eq_words(r)) and np.array_equal(host(c.build_eq(r, out=dev_view(eq * 0)[0])), eq)
        assert np.array_equal(c.mle_eval_batch(small, r), tref.py_eval(small, 32, r)) and np.array_equal(c.mle_eval_batch(sv, r), tref.py_eval(small, 32, r))
        assert np.array_equal(c.mle_fix_variables(small, r[:2]), tref.py_fix(small, r[:2]))
        assert np.array_equal(host(c.mle_fix_variables(sv, r[:2])), tref.py_fix(small, r[:2]))
        y = c.spmv_t(1, xs)
        rp, col, val = r1cs[1]
        for cc in (int(col[0]), int(col[n // 2]), int(col[n - 1])):
            rows = np.nonzero(col == cc)[0]
            assert np.array_equal(y[cc], pysum(ref.rmul(val[rows], xs[rows])))
        assert np.array_equal(host(c.spmv_t(1, dev_view(xs)[0])), y)
        # nothing else has moved
        assert np.array_equal(sc.prove_round(int(point[1])), msgs[2])
        assert np.array_equal(sc.prove_round(int(point[2])), msgs[3])
        assert np.array_equal(sc.final(int(point[3])), final)
        sc.end()
        if pending:
            c._chk(L().lfplus_rg_from_f(c.h, dp.b, dp.k, dp.l))            # collects the pass
        got = _rg_read(c, k, kappa, n)
        assert all(np.array_equal(g, x) for g, x in zip(got, want))
        assert np.array_equal(c.get_witness(), f)
        assert np.array_equal(c.spmv(1, xs)[:4], np.stack([ref.rmul(val[i], xs[col[i]]) for i in range(4)]).astype(np.uint64)), "the resident matrices"
    finally:
        c.close()
