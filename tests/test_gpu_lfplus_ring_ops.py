"""Ring arithmetic on arrays on the device (lfplus_ring_mul, lfplus_spmv and their _device forms, include/lfplus.h) against Python integers
(tests/lfplus_mlsumcheck_ref.rmul) on the small shapes and the oracle's lfp_ring_mul (tests/lfp.py) on the grid-stride case: both modes, partial and several
16-element groups, the accumulator bound at n_terms = 64, host and device memory, the in-place forms, the refusals in their stated order, and the independence
from everything else a context holds.  Bit-exact: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import lfp
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
P, D = plus.P, plus.D
E_ARG = plus.E_ARG
SENT = 0x5A5A5A5A5A5A5A5A
u64p = plus.u64p


def L():
    return plus._lib()


def err(ctx):
    return L().lfplus_last_error(ctx.h).decode()


def hp(a):
    return a.ctypes.data_as(u64p)


def dev_view(a):
    """the words of `a` as a view at a non-zero, 16-byte aligned offset of a larger device allocation -> (view, the whole allocation)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    whole = torch.full((a.size + 6,), SENT, dtype=torch.int64, device="cuda")
    view = whole[2:2 + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a.view(np.int64).copy()))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != whole.data_ptr()
    return view, whole


def host(t):
    return t.cpu().numpy().view(np.uint64)


def margins_intact(whole):
    w = host(whole)
    return (w[:2] == SENT).all() and (w[-4:] == SENT).all()


@pytest.fixture(scope="module")
def ctx():
    c = plus.PlusContext(0)      # BARE: no matrix, no witness
    yield c
    c.close()


# ---- inputs and the Python-integer reference ------------------------------------------------------------------------------------------------------------------------
def short_rows(seed, count):
    """short-challenge rows: coefficients in [-128, 128) mod p"""
    v = (lfp.splitmix(seed, 0, count * D) % np.uint64(256)).astype(np.int64) - 128
    return np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(count, D)


def edge_rows():
    """0, 1, all p - 1, X^15, a short-challenge row"""
    e = np.zeros((5, D), dtype=np.uint64)
    e[1, 0] = 1
    e[2] = P - 1
    e[3, 15] = 1
    e[4] = short_rows(0xE4, 1)[0]
    return e


def mixed_rows(seed, shape):
    """random canonical rows with the edge rows among them: row r (flat) is edge row (r + seed) % 7 when that is < 5"""
    rows = int(np.prod(shape))
    out = ref.rand_ring(seed, (rows, D)).copy()
    e = edge_rows()
    for r in range(rows):
        w = (r + seed) % 7
        if w < 5:
            out[r] = short_rows(seed * 131 + r, 1)[0] if w == 4 else e[w]
    return out.reshape(tuple(shape) + (D,))


def py_ring_mul(a, b, broadcast):
    """sum_i a_i * b_i in Python integers: a (T, count, 16); b (T, count, 16), or (T, 16) with broadcast"""
    acc = np.zeros(a.shape[1:], dtype=object)
    for i in range(a.shape[0]):
        acc = acc + ref.rmul(a[i], b[i][None, :] if broadcast else b[i])
    return (acc % P).astype(np.uint64)


# ---- against Python integers ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("n_terms", [1, 2, 3])
@pytest.mark.parametrize("count", [1, 15, 16, 17, 33])
def test_against_python_integers(ctx, count, n_terms, broadcast):
    seed = 0x100 + 16 * count + 2 * n_terms + int(broadcast)
    a = mixed_rows(seed, (n_terms, count))
    b = mixed_rows(seed + 3, (n_terms,) if broadcast else (n_terms, count))
    want = py_ring_mul(a, b, broadcast)
    a0, b0 = a.copy(), b.copy()
    got = ctx.ring_mul(a, b, broadcast=broadcast)
    assert np.array_equal(got, want)
    assert np.array_equal(a, a0) and np.array_equal(b, b0), "inputs are never written"
    if n_terms == 1:                                                            # the 2-d spelling of one term
        assert np.array_equal(ctx.ring_mul(a[0], b[0], broadcast=broadcast), want)
    if broadcast:                                                               # mode 1 is mode 0 with b replicated
        rep = np.ascontiguousarray(np.broadcast_to(b[:, None, :], a.shape))
        assert np.array_equal(ctx.ring_mul(a, rep), want)


def test_edge_rows_pairwise(ctx):
    """every edge row times every edge row (a partial second group), element-wise and as the coefficient of a broadcast; a square with a and b the same array"""
    e = edge_rows()
    a = np.repeat(e, 5, axis=0)
    b = np.tile(e, (5, 1))
    want = py_ring_mul(a[None], b[None], False)
    assert np.array_equal(ctx.ring_mul(a, b), want)
    for i in range(5):
        assert np.array_equal(ctx.ring_mul(e, e[i], broadcast=True), want.reshape(5, 5, D)[:, i])
    assert np.array_equal(ctx.ring_mul(a, a), py_ring_mul(a[None], a[None], False))
    x15sq = np.zeros(D, dtype=np.uint64)
    x15sq[14] = P - 1                                                           # X^15 X^15 = -X^14: the wrap sign
    assert np.array_equal(want.reshape(5, 5, D)[3, 3], x15sq)


@pytest.mark.parametrize("broadcast", [False, True])
def test_accumulator_bound(ctx, broadcast):
    """every word of both operands p - 1, n_terms = 64: coefficient 0 is the most negative lazy sum the envelope allows (15 * 64 subtracted products of
    (p - 1)^2), coefficient 15 the most positive (16 * 64 added)"""
    n_terms, count = 64, 17
    a = np.full((n_terms, count, D), P - 1, dtype=np.uint64)
    b = np.full((n_terms, D) if broadcast else (n_terms, count, D), P - 1, dtype=np.uint64)
    row = [((c + 1) - (15 - c)) * n_terms * (P - 1) * (P - 1) % P for c in range(D)]
    want = np.tile(np.array(row, dtype=object).astype(np.uint64), (count, 1))
    assert np.array_equal(want, py_ring_mul(a[:, :2], b if broadcast else b[:, :2], broadcast)[0][None].repeat(count, axis=0))
    assert np.array_equal(ctx.ring_mul(a, b, broadcast=broadcast), want)


@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("cap", [3, 1])
def test_the_block_cap_forces_the_grid_stride_loop(ctx, monkeypatch, cap, broadcast):
    """LFPLUS_RING_BLOCKS workgroups over 7 groups of 16: every workgroup takes a second pass, the last group is a tail of 5.  Reference: the oracle"""
    monkeypatch.setenv("LFPLUS_RING_BLOCKS", str(cap))
    n_terms, count = 2, 6 * 16 + 5
    a = ref.rand_ring(0x6A + cap, (n_terms, count, D))
    b = ref.rand_ring(0x6B + cap, (n_terms, D) if broadcast else (n_terms, count, D))
    want = np.zeros((count, D), dtype=np.uint64)
    for i in range(n_terms):
        for x in range(count):
            want[x] = lfp.addmod(want[x], lfp.ring_mul(a[i, x], b[i] if broadcast else b[i, x]))
    assert np.array_equal(ctx.ring_mul(a, b, broadcast=broadcast), want)
    av, aw = dev_view(a)
    if broadcast:
        got = ctx.ring_mul(av, b, broadcast=True)
    else:
        bv, bw = dev_view(b)
        got = ctx.ring_mul(av, bv)
    assert np.array_equal(host(got), want)


# ---- the device form ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("n_terms,count", [(1, 17), (3, 33)])
def test_device_arrays_give_the_host_words_and_are_not_written(ctx, n_terms, count, broadcast):
    a = mixed_rows(0x300 + count, (n_terms, count))
    b = mixed_rows(0x301 + count, (n_terms,) if broadcast else (n_terms, count))
    want = ctx.ring_mul(a, b, broadcast=broadcast)
    assert np.array_equal(want, py_ring_mul(a, b, broadcast))
    av, aw = dev_view(a)
    ov, ow = dev_view(np.full((count, D), SENT, dtype=np.uint64))
    if broadcast:
        got = ctx.ring_mul(av, b, broadcast=True, out=ov)
    else:
        bv, bw = dev_view(b)
        got = ctx.ring_mul(av, bv, out=ov)
        assert np.array_equal(host(bv), b) and margins_intact(bw)
    assert got is ov and np.array_equal(host(ov), want)
    assert np.array_equal(host(av), a) and margins_intact(aw) and margins_intact(ow)


@pytest.mark.parametrize("count", [16, 37])
def test_in_place_forms(ctx, count):
    """out is a with one term in both modes, out is b element-wise: the words of the out-of-place call, in both memory spaces"""
    a, b = mixed_rows(0x400 + count, (count,)), mixed_rows(0x401 + count, (count,))
    coef = short_rows(0x402, 1)[0]
    want0, want1, wantsq = py_ring_mul(a[None], b[None], False), py_ring_mul(a[None], coef[None], True), py_ring_mul(a[None], a[None], False)
    for dev in (False, True):
        def fresh(x):
            return dev_view(x)[0] if dev else x.copy()

        def words(x):
            return host(x) if dev else x
        x, y = fresh(a), fresh(b)
        assert ctx.ring_mul(x, y, out=x) is x and np.array_equal(words(x), want0) and np.array_equal(words(y), b)
        x, y = fresh(a), fresh(b)
        assert ctx.ring_mul(x, y, out=y) is y and np.array_equal(words(y), want0) and np.array_equal(words(x), a)
        x = fresh(a)
        assert ctx.ring_mul(x, coef, broadcast=True, out=x) is x and np.array_equal(words(x), want1)
        x = fresh(a)
        assert ctx.ring_mul(x, x, out=x) is x and np.array_equal(words(x), wantsq)      # a square onto itself


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def rm(ctx, a, b, n_terms, count, mode, out):
    return L().lfplus_ring_mul(ctx.h, a, b, n_terms, count, mode, out)


def rmd(ctx, a, b, n_terms, count, mode, out):
    return L().lfplus_ring_mul_device(ctx.h, C.c_void_p(a), C.c_void_p(b), n_terms, count, mode, C.c_void_p(out))


def test_refusals_in_their_stated_order(ctx):
    count = 20
    a, b = ref.rand_ring(0x51, (2, count, D)), ref.rand_ring(0x52, (2, count, D))
    out = np.full((count, D), SENT, dtype=np.uint64)
    pa, pb, po = hp(a), hp(b), hp(out)
    sharded = plus.PlusContext(0)
    try:
        sharded.set_sharding_model(0, 2)
        # a NULL array, before the envelope
        for args in ((None, pb, po), (pa, None, po), (pa, pb, None)):
            assert rm(ctx, args[0], args[1], 0, count, 0, args[2]) == E_ARG and "null" in err(ctx)
        assert rmd(ctx, None, None, 0, count, 0, None) == E_ARG and "null" in err(ctx)
        # the envelope, before the sharded context
        for c in (ctx, sharded):
            for nt, cnt, mode in ((0, count, 0), (65, count, 0), (2, 0, 0), (2, (1 << 28) + 1, 0), (2, count, 2), (2, count, -1)):
                assert rm(c, pa, pb, nt, cnt, mode, po) == E_ARG and "envelope" in err(c), (nt, cnt, mode)
        # the sharded context, before the overlap rules
        assert rm(sharded, pa, pb, 2, count, 0, po) == E_ARG and "sharded" in err(sharded)
        assert rm(sharded, pa, pb, 2, count, 0, pa) == E_ARG and "sharded" in err(sharded)
        assert rmd(sharded, a.ctypes.data, b.ctypes.data, 2, count, 0, out.ctypes.data) == E_ARG and "sharded" in err(sharded)
        # overlap: out exactly a with two terms, partial overlaps, out inside b, the coefficients of a broadcast
        a_before = a.copy()
        one = 16 * 8
        for o_addr, mode, nt in ((a.ctypes.data, 0, 2), (a.ctypes.data + one, 0, 1), (a.ctypes.data + 8, 0, 1), (b.ctypes.data + one * count, 0, 2),
                                 (b.ctypes.data, 1, 1), (a.ctypes.data + one * (2 * count - 1), 0, 2)):
            assert rm(ctx, pa, pb, nt, count, mode, C.cast(C.c_void_p(o_addr), u64p)) == E_ARG and "overlaps" in err(ctx), (o_addr, mode, nt)
        # ... before the pointer checks: host addresses in the device form
        assert rmd(ctx, a.ctypes.data, b.ctypes.data, 2, count, 0, a.ctypes.data) == E_ARG and "overlaps" in err(ctx)
        assert np.array_equal(a, a_before) and (out == SENT).all()
    finally:
        sharded.close()


def test_device_pointer_refusals(ctx):
    count = 24
    a, b = ref.rand_ring(0x53, (1, count, D)), ref.rand_ring(0x54, (1, count, D))
    av, aw = dev_view(a)
    bv, bw = dev_view(b)
    ov, ow = dev_view(np.full((count, D), SENT, dtype=np.uint64))
    torch.cuda.empty_cache()
    big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")      # an allocation of its own (requested from an empty cache)
    pinned = torch.zeros((count, D), dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    coef = np.ascontiguousarray(b[0, 0])
    pageable = np.zeros((count, D), dtype=np.uint64)
    good = (av.data_ptr(), bv.data_ptr(), ov.data_ptr())
    # (the misaligned pointer is the slot's own array + 8: as `out` it must not overlap an input, or the overlap rule answers first)
    bad = [("pinned host memory", lambda slot: pinned.data_ptr()), ("pageable host memory", lambda slot: pageable.ctypes.data), ("dev + 8", lambda slot: good[slot] + 8),
           ("off the end", lambda slot: big.data_ptr() + (32 << 20) - 128)]
    for name, addr in bad:
        for slot in range(3):
            args = list(good)
            args[slot] = addr(slot)
            assert rmd(ctx, args[0], args[1], 1, count, 0, args[2]) == E_ARG and "device memory" in err(ctx), (name, slot)
        # mode 1: b is a host pointer and is not looked up; a bad array is refused BEFORE the words of b are tested
        badcoef = coef.copy()
        badcoef[3] = P
        assert rmd(ctx, addr(0), badcoef.ctypes.data, 1, count, 1, good[2]) == E_ARG and "device memory" in err(ctx), name
        assert rmd(ctx, good[0], coef.ctypes.data, 1, count, 1, addr(2)) == E_ARG and "device memory" in err(ctx), name
    assert (host(ov) == SENT).all() and np.array_equal(host(av), a) and np.array_equal(host(bv), b)
    # the same arrays, well-formed
    assert rmd(ctx, *good[:2], 1, count, 0, good[2]) == 0 and np.array_equal(host(ov), py_ring_mul(a, b, False))
    assert rmd(ctx, good[0], coef.ctypes.data, 1, count, 1, good[2]) == 0 and np.array_equal(host(ov), py_ring_mul(a, coef[None], True))


@pytest.mark.parametrize("word", [P, 2**64 - 1])
def test_non_canonical_words(ctx, word):
    n_terms, count = 2, 19
    a, b = ref.rand_ring(0x55, (n_terms, count, D)), ref.rand_ring(0x56, (n_terms, count, D))
    coef = ref.rand_ring(0x57, (n_terms, D))
    out = np.full((count, D), SENT, dtype=np.uint64)
    for where in ((0, 0, 0), (n_terms - 1, count - 1, D - 1)):
        for which in ("a", "b"):
            x, y = a.copy(), b.copy()
            (x if which == "a" else y)[where] = word
            assert rm(ctx, hp(x), hp(y), n_terms, count, 0, hp(out)) == E_ARG and "non-canonical" in err(ctx), (where, which)
            xv, xw = dev_view(x)
            yv, yw = dev_view(y)
            ov, ow = dev_view(out)
            ctx.wait_stream()
            assert rmd(ctx, xv.data_ptr(), yv.data_ptr(), n_terms, count, 0, ov.data_ptr()) == E_ARG and "non-canonical" in err(ctx), (where, which)
            assert margins_intact(ow)
        x = a.copy()
        x[where] = word
        assert rm(ctx, hp(x), hp(coef), n_terms, count, 1, hp(out)) == E_ARG and "non-canonical word in a" in err(ctx)
        cw = coef.copy()
        cw[where[0], where[2]] = word
        assert rm(ctx, hp(a), hp(cw), n_terms, count, 1, hp(out)) == E_ARG and "in b" in err(ctx)
        assert rm(ctx, hp(x), hp(cw), n_terms, count, 1, hp(out)) == E_ARG and "in b" in err(ctx), "b is tested on the host, before the O(n) words"
    assert (out == SENT).all(), "the host out is untouched"
    assert np.array_equal(ctx.ring_mul(a, b), py_ring_mul(a, b, False)), "the context stays usable"


# ---- lfplus_spmv ----------------------------------------------------------------------------------------------------------------------------------------------------
def spmv_matrices(n):
    """a matrix with ring coefficients and one with constant coefficients: rows with 0, 1 and 5 non-zeros, a repeated column inside a row"""
    rng = np.random.default_rng(0x5B)
    nnz = np.array([(0, 1, 5)[r % 3] for r in range(n)])
    rowptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.uint32)
    col = rng.integers(0, n, size=int(rowptr[-1])).astype(np.uint32)
    col[rowptr[2] + 3] = col[rowptr[2] + 1]                                      # row 2 has five entries: two of them in one column
    ring = ref.rand_ring(0x5C, (col.size, D))
    const = np.zeros((col.size, D), dtype=np.uint64)
    const[:, 0] = ref.rand_ring(0x5D, (col.size,))
    return [(rowptr, col, ring), (rowptr, col.copy(), const)]


def py_spmv(mat, x):
    rowptr, col, val = mat
    out = np.zeros((rowptr.size - 1, D), dtype=object)
    for r in range(rowptr.size - 1):
        for k in range(rowptr[r], rowptr[r + 1]):
            out[r] = out[r] + ref.rmul(val[k], x[col[k]])
    return (out % P).astype(np.uint64)


def test_spmv_against_python_integers():
    n = 64
    mats = spmv_matrices(n)
    x = mixed_rows(0x5E, (n,))
    c = plus.PlusContext(0)
    try:
        y = np.full((n, D), SENT, dtype=np.uint64)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, hp(y)) == E_ARG and "no resident matrices" in err(c)
        c.set_matrices(mats, n=n)
        xv, xw = dev_view(x)
        for j, m in enumerate(mats):
            want = py_spmv(m, x)
            got = c.spmv(j, x)
            assert np.array_equal(got, want), j
            assert not want[0].any() and not want[3].any(), "rows without a non-zero"
            yv, yw = dev_view(y)
            assert c.spmv(j, xv, out=yv) is yv and np.array_equal(host(yv), want) and margins_intact(yw)
        assert np.array_equal(host(xv), x) and margins_intact(xw)
        # refusals: j out of range, a wrong n, overlap, a NULL array, device pointers, a non-canonical word
        assert L().lfplus_spmv(c.h, 2, hp(x), n, hp(y)) == E_ARG and "matrix 2 of 2" in err(c)
        assert L().lfplus_spmv(c.h, 0, hp(x), n - 1, hp(y)) == E_ARG and "wide" in err(c)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, None) == E_ARG and "null" in err(c)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, hp(x)) == E_ARG and "overlaps" in err(c)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, C.cast(C.c_void_p(x.ctypes.data + (n - 1) * D * 8), u64p)) == E_ARG and "overlaps" in err(c)
        assert L().lfplus_spmv_device(c.h, 0, C.c_void_p(xv.data_ptr()), n, C.c_void_p(xv.data_ptr() + D * 8)) == E_ARG and "overlaps" in err(c)
        yv, yw = dev_view(y)
        torch.cuda.empty_cache()
        big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")      # an allocation of its own (requested from an empty cache)
        torch.cuda.synchronize()
        off_end = big.data_ptr() + (32 << 20) - 128
        for px, py in ((x.ctypes.data, yv.data_ptr()), (xv.data_ptr() + 8, yv.data_ptr()), (xv.data_ptr(), y.ctypes.data), (xv.data_ptr(), yv.data_ptr() + 8),
                       (xv.data_ptr(), off_end), (off_end, yv.data_ptr())):
            assert L().lfplus_spmv_device(c.h, 0, C.c_void_p(px), n, C.c_void_p(py)) == E_ARG and "device memory" in err(c)
        assert (host(yv) == SENT).all()
        for pos, word in (((0, 0), P), ((n - 1, D - 1), 2**64 - 1)):
            bad = x.copy()
            bad[pos] = word
            assert L().lfplus_spmv(c.h, 0, hp(bad), n, hp(y)) == E_ARG and "non-canonical" in err(c)
            bv, bw = dev_view(bad)
            c.wait_stream()
            assert L().lfplus_spmv_device(c.h, 0, C.c_void_p(bv.data_ptr()), n, C.c_void_p(yv.data_ptr())) == E_ARG and "non-canonical" in err(c)
        assert (y == SENT).all(), "the host y is untouched"
        assert np.array_equal(c.spmv(1, x), py_spmv(mats[1], x)), "the context stays usable"
        sharer = plus.PlusContext(0)
        try:
            sharer.share_matrices(c)
            assert np.array_equal(sharer.spmv(0, x), py_spmv(mats[0], x))
        finally:
            sharer.close()
    finally:
        c.close()


def test_spmv_on_a_sharded_context_is_refused():
    n = 64
    x, y = ref.rand_ring(0x5F, (n, D)), np.full((n, D), SENT, dtype=np.uint64)
    c = plus.PlusContext(0)
    try:
        c.set_sharding_model(0, 2)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, hp(y)) == E_ARG and "no resident matrices" in err(c)      # (the state checks come first)
        c.set_matrices(spmv_matrices(n), n=n)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, hp(y)) == E_ARG and "sharded" in err(c)
        assert (y == SENT).all()
    finally:
        c.close()


# ---- independence ---------------------------------------------------------------------------------------------------------------------------------------------------
def _rg_read(c, k, kappa, n):
    Df, com = np.zeros((k, n, D), dtype=np.int8), np.zeros((k, kappa, D, D), dtype=np.uint64)
    tau, mt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int8)
    cs = [np.zeros((kappa, D), dtype=np.uint64) for _ in range(3)]
    c._chk(L().lfplus_rg_read(c.h, Df.ctypes.data_as(plus.i8p), hp(com), hp(tau), mt.ctypes.data_as(plus.i8p), *[hp(x) for x in cs]))
    return [Df, com, tau, mt] + cs


@pytest.mark.parametrize("pending", [False, True])
def test_a_loaded_context_is_not_disturbed(pending):
    """a matrix, a witness, a from_f pass (pending on the second stream or collected) and a generic sumcheck in its second round: ring_mul and spmv in between
    change none of the words that come out afterwards"""
    n, kappa, k = 1 << 15, 1, 2                                               # (from_f needs n > kappa k d l d)
    dp = plus.DecompParameters.for_frog(k)
    A = lfp.splitmix(1, 0, kappa * n * D).reshape(kappa, n, D) % np.uint64(P)
    v = (lfp.splitmix(2, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    f = np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)
    r1cs = [ref.rand_csr(0x55 + q, n, 1) for q in range(3)]
    tables, terms, degree, msgs, point, final = ref.case("b", 4)
    a, b = mixed_rows(0x71, (2, 33)), mixed_rows(0x72, (2, 33))
    xs = ref.rand_ring(0x73, (n, D))
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
        assert np.array_equal(c.ring_mul(a, b), py_ring_mul(a, b, False))
        assert np.array_equal(c.ring_mul(a, b[:, 0], broadcast=True), py_ring_mul(a, b[:, 0], True))
        y = c.spmv(1, xs)
        rows = [0, 1, n // 2, n - 1]
        rp, col, val = r1cs[1]
        assert all(np.array_equal(y[r], ref.rmul(val[r], xs[col[r]]).astype(np.uint64)) for r in rows)
        xv, xw = dev_view(xs)
        assert np.array_equal(host(c.spmv(1, xv)), y)
        av, aw = dev_view(a)
        assert np.array_equal(host(c.ring_mul(av, b[:, 0], broadcast=True)), py_ring_mul(a, b[:, 0], True))
        # nothing else has moved
        assert np.array_equal(sc.prove_round(int(point[1])), msgs[2])
        assert np.array_equal(sc.prove_round(int(point[2])), msgs[3])
        assert np.array_equal(sc.final(int(point[3])), final)
        sc.end()
        if pending:
            c._chk(L().lfplus_rg_from_f(c.h, dp.b, dp.k, dp.l))            # collects the pass
        got = _rg_read(c, k, kappa, n)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert np.array_equal(c.get_witness(), f)
    finally:
        c.close()


# ---- the use the calls exist for ------------------------------------------------------------------------------------------------------------------------------------
def test_r1cs_residual_from_the_witness_on_the_device():
    """the smallest workload ComR1CS accepts, k = 1: g_q = spmv(q, f) on the device, ring_mul(g_0, g_1) is g_2 word for word on a satisfied instance; with one
    witness coefficient changed the first row where they differ is the first_bad of lfplus_r1cs_check"""
    n, B = 64, 8
    r1cs = plus.r1cs_decomposed_square((plus.identity_csr(n),) * 3, n, B, 1)
    z = np.zeros((n, D), dtype=np.uint64)
    z[:, 0] = lfp.splitmix(0x81, 0, n) >> np.uint64(63)                          # 0 / 1 constants: z o z = z
    c = plus.PlusContext(0)
    try:
        c.set_matrix(ref.rand_ring(0x82, (1, n, D)))
        c.set_matrices(r1cs)
        for f, bad_row in ((z, None), (None, 37)):
            if f is None:
                f = z.copy()
                f[bad_row, 0] = 2                                                # 2 * 2 != 2
                f[bad_row + 9, 3] = 1                                            # (a later row fails as well)
            c.set_witness(f)
            ok, failed, first_bad, _ = c.r1cs_check(None)
            fv, fw = dev_view(f)
            g = [c.spmv(q, fv) for q in range(3)]
            prod = host(c.ring_mul(g[0], g[1]))
            g2 = host(g[2])
            differ = np.nonzero((prod != g2).any(axis=1))[0]
            if bad_row is None:
                assert ok and first_bad == n and differ.size == 0 and np.array_equal(prod, g2)
            else:
                assert not ok and failed & plus.REL_R1CS and differ.size == 2 and differ[0] == first_bad == bad_row
            assert np.array_equal(host(fv), f) and margins_intact(fw)
    finally:
        c.close()
