"""Gadget maps on arrays on the device (lfplus_balanced_decompose, lfplus_balanced_recompose, lfplus_linf_norm, their _device forms and
lfplus_set_matrices_gadget, include/lfplus.h) against Python integers (tests/lfplus_digits_ref.py) and against the calls of the library that already cut digits
or load matrices: host and device memory, both layouts, the refusals in their stated order.  Bit-exact: no tolerance.

Shapes.  A thread owns one word and a workgroup 256 of them (16 elements); LFPLUS_DIGIT_BLOCKS caps the grid (default 2048).  With the cap at 256 one pass of the
grid covers 4096 elements, so count = 4097 is one element past a grid-stride boundary; 257 is one past a multiple of the workgroup, 3 less than a wave.
  The cross-check with lfplus_rg_read runs at n = 2^15, not at 256: lfplus_rg_from_f refuses n <= kappa k d l d (LFPLUS_E_SMALL_N; 16896 for kappa = 1, k = 3 and
the l = 22 of the Frog parameters), and 2^15 is the smallest power of two above it -- the size the other from_f tests of this suite use."""
import ctypes as C

import numpy as np
import pytest
import torch

import lfp
import lfplus_digits_ref as dref
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus
from test_gpu_lfplus_ring_ops import _rg_read, dev_view, host, margins_intact

pytestmark = pytest.mark.gpu
P, D = plus.P, plus.D
E_ARG = plus.E_ARG
SENT = 0x5A5A5A5A5A5A5A5A
u64p = plus.u64p
GADGET, PLANES = plus.DIGITS_GADGET, plus.DIGITS_PLANES
BK = [(2, 1), (2, 64), (3, 40), (14, 16), (2**31, 2), (10**9 + 7, 3), (2**62, 2)]


def L():
    return plus._lib()


def err(ctx):
    return L().lfplus_last_error(ctx.h).decode()


def hp(a):
    return a.ctypes.data_as(u64p)


def at(addr):
    return C.cast(C.c_void_p(addr), u64p)


@pytest.fixture(scope="module")
def ctx():
    c = plus.PlusContext(0)      # BARE: no matrix, no witness
    yield c
    c.close()


# ---- decompose and recompose against Python integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 257, 4097])
@pytest.mark.parametrize("b,k", BK, ids=[f"b{b}-k{k}" for b, k in BK])
def test_decompose_and_recompose_against_the_reference(ctx, monkeypatch, b, k, count):
    monkeypatch.setenv("LFPLUS_DIGIT_BLOCKS", "256")
    x = dref.operands(0x100 + 7 * k + count, count, b, k)
    x0 = x.copy()
    kept = dref.kept(x, b, k)
    xv, xw = dev_view(x)
    for layout in (GADGET, PLANES):
        want = dref.decompose(x, b, k, layout)
        got = ctx.balanced_decompose(x, b, k, layout)
        assert got.shape == (count * k, D) and np.array_equal(got, want), (b, k, count, layout)
        ov, ow = dev_view(np.full((count * k, D), SENT, dtype=np.uint64))
        assert ctx.balanced_decompose(xv, b, k, layout, out=ov) is ov
        assert np.array_equal(host(ov), got) and margins_intact(ow), "the device form writes the words of the host form and nothing else"
        back = ctx.balanced_recompose(got, b, k, layout)
        assert back.shape == (count, D) and np.array_equal(back, kept), (b, k, count, layout)
        bv, bw = dev_view(np.full((count, D), SENT, dtype=np.uint64))
        assert ctx.balanced_recompose(ov, b, k, layout, out=bv) is bv
        assert np.array_equal(host(bv), back) and margins_intact(bw) and np.array_equal(host(ov), got)
    assert np.array_equal(x, x0) and np.array_equal(host(xv), x) and margins_intact(xw), "inputs are never written"
    u, inv = np.unique(x, return_inverse=True)
    fits = np.array([dref.digits(int(v), b, k)[1] == 0 for v in u])[inv.reshape(-1)].reshape(x.shape)
    assert np.array_equal(kept[fits], x[fits]), "recompose inverts decompose exactly where the value fitted"


@pytest.mark.parametrize("layout", [GADGET, PLANES])
def test_recompose_of_general_elements(ctx, layout):
    """random words up to p - 1 in every slot, k = 64, b = 2^62: the 160-bit lazy sum at its longest, against Python integers; one element of p - 1 throughout"""
    b, k, count = 2**62, 64, 19
    x = ref.rand_ring(0x2A + layout, (count * k, D)).copy()
    sel = np.arange(k) * (1 if layout == GADGET else count) + (5 * k if layout == GADGET else 5)
    x[sel] = P - 1                                                              # element 5: every digit slot p - 1
    want = dref.recompose(x, b, k, layout)
    assert np.array_equal(want[5], np.full(D, (P - 1) * sum(pow(b, i, P) for i in range(k)) % P, dtype=np.uint64))
    x0 = x.copy()
    assert np.array_equal(ctx.balanced_recompose(x, b, k, layout), want) and np.array_equal(x, x0)
    xv, xw = dev_view(x)
    assert np.array_equal(host(ctx.balanced_recompose(xv, b, k, layout)), want) and np.array_equal(host(xv), x) and margins_intact(xw)


# ---- cross-checks with the calls that already cut digits ------------------------------------------------------------------------------------------------------------
def _commitment(n, kappa=1, seed=1):
    return lfp.splitmix(seed, 0, kappa * n * D).reshape(kappa, n, D) % np.uint64(P)


@pytest.mark.parametrize("b,k", [(2, 4), (2**31, 2)])
def test_gadget_order_is_what_witness_from_z_makes_resident(ctx, b, k):
    m = 64
    z = dref.operands(0x31 + k, m, b, k)
    c = plus.PlusContext(0)
    try:
        c.set_matrix(_commitment(m * k))
        c.witness_from_z(z, b, k)
        f = c.get_witness()
        assert np.array_equal(ctx.balanced_decompose(z, b, k, GADGET), f)
        assert np.array_equal(c.balanced_decompose(z, b, k, GADGET), f) and np.array_equal(c.get_witness(), f), "on the loaded context, whose witness stays"
        assert np.array_equal(host(ctx.balanced_decompose(dev_view(z)[0], b, k, GADGET)), f)
    finally:
        c.close()


@pytest.mark.parametrize("B", [2**16, 10**9 + 7])
def test_planes_with_two_digits_are_the_halves_of_lfplus_decompose(ctx, B):
    n = 64
    f = dref.operands(0x41, n, B, 2)
    r = ref.rand_ring(0x42, (6, 2, D))
    c = plus.PlusContext(0)
    try:
        out = c.decompose(f, _commitment(n), B, r)
        planes = ctx.balanced_decompose(f, B, 2, PLANES)
        assert np.array_equal(planes[:n], out["F0"]) and np.array_equal(planes[n:], out["F1"])
    finally:
        c.close()


def test_planes_are_the_digit_order_of_lfplus_rg_read(ctx):
    """(b, k) = (4, 3): plane i of layout 1 is D_f[i] of the range check's from_f, digit by digit (as centred int8 there, as canonical residues here)"""
    n, kappa, b, k = 1 << 15, 1, 4, 3
    dp = plus.DecompParameters.for_frog(k, b)
    v = (lfp.splitmix(0x51, 0, n * D) % np.uint64(b**k)).astype(np.int64) - (b**k) // 2      # centred values that fit k digits, both ends included
    f = np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)
    c = plus.PlusContext(0)
    try:
        c.set_matrix(_commitment(n, kappa))
        c.set_witness(f)
        c._chk(L().lfplus_rg_from_f(c.h, dp.b, dp.k, dp.l))
        Df = _rg_read(c, k, kappa, n)[0].astype(np.int64)
        planes = ctx.balanced_decompose(f, b, k, PLANES).reshape(k, n, D)
        assert np.array_equal(planes, np.where(Df < 0, np.uint64(P) - (-Df).astype(np.uint64), Df.astype(np.uint64)))
        assert np.array_equal(ctx.balanced_recompose(planes.reshape(k * n, D), b, k, PLANES), f)
    finally:
        c.close()


# ---- linf_norm ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_linf_norm_is_the_absmax_of_the_relation_checks(ctx):
    n, kappa = 64, 1
    f = dref.operands(0x61, n, 3, 8)
    f[f > np.uint64(2**40)] %= np.uint64(1 << 20)                                # a vector whose largest entry is not a corner
    f[17, 3] = P - 123456789
    c = plus.PlusContext(0)
    try:
        c.set_matrix(_commitment(n, kappa))
        c.set_witness(f)
        r = ref.rand_ring(0x62, (6, 2, D))
        _, _, absmax = c.linb_check(None, r, np.zeros((1, 2, D), dtype=np.uint64))
        assert absmax == 123456789 == dref.linf(f)
        assert ctx.linf_norm(f) == absmax and c.linf_norm(f) == absmax
        fv, fw = dev_view(f)
        assert ctx.linf_norm(fv) == absmax and np.array_equal(host(fv), f) and margins_intact(fw)
    finally:
        c.close()


@pytest.mark.parametrize("planted", [(P - 1) // 2, (P + 1) // 2])
def test_linf_norm_finds_a_single_planted_word(ctx, planted):
    """count = 2048 * 8 * 16 + 5 elements: 2048 workgroups of 256 threads stride eight times and leave a tail of 80 words to the first one"""
    count = 2048 * 8 * 16 + 5
    base = (lfp.splitmix(0x63, 0, count * D) % np.uint64(1000)).reshape(count, D)
    xv = torch.from_numpy(base.view(np.int64).copy()).cuda()
    assert ctx.linf_norm(xv) == 999 == ctx.linf_norm(base)
    flat = xv.view(-1)
    for word in (0, count * D - 1, count * D - 80 + 3):
        old = int(flat[word])
        flat[word] = int(np.array(planted, dtype=np.uint64).view(np.int64))
        assert ctx.linf_norm(xv) == (P - 1) // 2, word
        flat[word] = old
    assert ctx.linf_norm(xv) == 999


# ---- set_matrices_gadget --------------------------------------------------------------------------------------------------------------------------------------------
def _ragged(seed, rows, m, const):
    rng = np.random.default_rng(seed)
    nnz = np.array([(0, 1, 5, 2)[(r + seed) % 4] for r in range(rows)])
    rowptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.uint32)
    col = rng.integers(0, m, size=int(rowptr[-1])).astype(np.uint32)
    val = np.zeros((col.size, D), dtype=np.uint64)
    if const:
        val[:, 0] = ref.rand_ring(seed + 1, (col.size,))
    else:
        val[:] = ref.rand_ring(seed + 1, (col.size, D))
    return rowptr, col, val


def _heavy(seed, rows, m):
    """two entries of every row in column 1 (2 rows > 64 entries: the workgroup path of lfplus_spmv_t), one in a random column"""
    rng = np.random.default_rng(seed)
    col = np.stack([np.full(rows, 1), rng.integers(0, m, size=rows), np.full(rows, 1)], axis=1).reshape(-1).astype(np.uint32)
    val = np.zeros((col.size, D), dtype=np.uint64)
    val[:, 0] = ref.rand_ring(seed + 1, (col.size,))
    return np.arange(0, 3 * rows + 1, 3, dtype=np.uint32), col, val


def _system(kind, n, m):
    if kind == "identity":
        return [plus.identity_csr(m) for _ in range(3)], m
    rows = min(n, m + 3)
    if kind == "ragged":
        return [_ragged(0x70 + q, rows, m, const=False) for q in range(3)], rows
    return [_heavy(0x80, n, m), _ragged(0x81, n, m, const=True), _ragged(0x82, n, m, const=True)], n      # (every row of the square: 2 n entries in column 1)


def _r1cs_linearize(c, n):
    nvars = n.bit_length() - 1
    msgs, ro, ev = np.zeros((nvars, 4, D), dtype=np.uint64), np.zeros(nvars, dtype=np.uint64), np.zeros((4, D), dtype=np.uint64)
    tr = plus.PoseidonTranscript()                                              # (held in a name: the object frees its handle when it is collected)
    c._chk(L().lfplus_r1cs_linearize(c.h, tr.h, None, None, None, hp(msgs), hp(ro), hp(ev)))
    return msgs, ro, ev


@pytest.mark.parametrize("kind", ["identity", "ragged", "heavy"])
@pytest.mark.parametrize("b", [2, 3])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n", [64, 1024])
def test_set_matrices_gadget_is_the_host_built_decomposed_square(n, k, b, kind):
    m = n // k
    short, rows = _system(kind, n, m)
    assert kind != "heavy" or np.bincount(short[0][1], minlength=m)[1] > 64
    before = [tuple(a.copy() for a in mat) for mat in short]
    square = plus.r1cs_decomposed_square(short, n, b, k)
    if kind == "identity":                                                      # a satisfied system: z of 0 / 1 constants, f its digits
        z = np.zeros((m, D), dtype=np.uint64)
        z[:, 0] = lfp.splitmix(0x90, 0, m) % np.uint64(2)
        f = plus.gadget_decompose(z, b, k)
    else:
        f = ref.rand_ring(0x91, (n, D))
    x, v = ref.rand_ring(0x92, (n, D)), ref.rand_ring(0x93, (n, D))
    A = _commitment(n)
    shape = plus.CCSShape(3, [[0, 1, 2], [2]], [1, -1])                         # degree 3
    twin, g, sharer = plus.PlusContext(0), plus.PlusContext(0), plus.PlusContext(0)
    try:
        outs = []
        for c in (twin, g):
            c.set_matrix(A)
            if c is twin:
                c.set_matrices(square, n=n)
            else:
                c.set_matrices_gadget(short, m, b, k)
            c.set_witness(f)
            o = [c.spmv(j, x) for j in range(3)] + [c.spmv_t(j, v) for j in range(3)]
            o += list(c.r1cs_check(None)) + list(_r1cs_linearize(c, n))
            linb, proof = plus.ComCCS(shape, None, None, None, c).linearize(c, plus.PoseidonTranscript(), resident=True)
            outs.append(o + [proof["msgs"], proof["r"], proof["evals"]])
        assert len(outs[0]) == len(outs[1]) == 16
        for i, (a, bb) in enumerate(zip(*outs)):
            assert np.array_equal(a, bb), i
        assert outs[0][6] == (kind == "identity"), "the identity system is satisfied, the random witnesses are not"
        assert all(np.array_equal(x_, y_) for mat, old in zip(short, before) for x_, y_ in zip(mat, old)), "the short arrays are never written"
        # the set is reference-counted like any other: a sharer outlives the context that loaded it
        sharer.share_matrices(g)
        g.close()
        for j in range(3):
            assert np.array_equal(sharer.spmv(j, x), outs[0][j]) and np.array_equal(sharer.spmv_t(j, v), outs[0][3 + j])
    finally:
        for c in (twin, g, sharer):
            c.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def dec(c, i, count, b, k, layout, o):
    return L().lfplus_balanced_decompose(c.h, i, count, b, k, layout, o)


def rec(c, i, count, b, k, layout, o):
    return L().lfplus_balanced_recompose(c.h, i, count, b, k, layout, o)


def decd(c, i, count, b, k, layout, o):
    return L().lfplus_balanced_decompose_device(c.h, i, count, b, k, layout, o)


def recd(c, i, count, b, k, layout, o):
    return L().lfplus_balanced_recompose_device(c.h, i, count, b, k, layout, o)


def test_refusals_of_the_array_calls_in_their_stated_order(ctx):
    count, b, k = 20, 3, 4
    x = ref.rand_ring(0xA1, (count * k, D))
    out = np.full((count * k, D), SENT, dtype=np.uint64)
    am = C.c_uint64(SENT)
    px, po = hp(x), hp(out)
    sharded = plus.PlusContext(0)
    try:
        sharded.set_sharding_model(0, 2)
        for f in (dec, rec):
            # a NULL array, before the envelope
            assert f(ctx, None, count, 1, k, 0, po) == E_ARG and "null" in err(ctx)
            assert f(ctx, px, count, b, 0, 0, None) == E_ARG and "null" in err(ctx)
            # the envelope, before the sharded context
            for c in (ctx, sharded):
                for cnt, bb, kk, lay in ((0, b, k, 0), ((1 << 28) // k + 1, b, k, 0), (count, b, 0, 0), (count, b, 65, 0), (count, 1, k, 0), (count, 0, k, 0),
                                         (count, 2**62 + 1, k, 0), (count, b, k, 2), (count, b, k, -1), ((1 << 28) + 1, b, 1, 1)):
                    assert f(c, px, cnt, bb, kk, lay, po) == E_ARG and "envelope" in err(c), (cnt, bb, kk, lay)
            # the sharded context, before the overlap
            assert f(sharded, px, count, b, k, 0, po) == E_ARG and "sharded" in err(sharded)
            assert f(sharded, px, count, b, k, 0, px) == E_ARG and "sharded" in err(sharded)
        for f in (decd, recd):
            assert f(ctx, None, count, b, k, 0, None) == E_ARG and "null" in err(ctx)
            assert f(sharded, x.ctypes.data, count, b, k, 0, out.ctypes.data) == E_ARG and "sharded" in err(sharded)
        assert L().lfplus_linf_norm(ctx.h, None, count, C.byref(am)) == E_ARG and "null" in err(ctx)
        assert L().lfplus_linf_norm(ctx.h, px, count, None) == E_ARG and "null" in err(ctx)
        for c in (ctx, sharded):
            for cnt in (0, (1 << 28) + 1):
                assert L().lfplus_linf_norm(c.h, px, cnt, C.byref(am)) == E_ARG and "envelope" in err(c)
        assert L().lfplus_linf_norm(sharded.h, px, count, C.byref(am)) == E_ARG and "sharded" in err(sharded)
        assert L().lfplus_linf_norm_device(sharded.h, x.ctypes.data, count, C.byref(am)) == E_ARG and "sharded" in err(sharded)
        # out overlapping in in any way: exactly, by one element, by one word, the last element of the larger side; before the pointer checks of the device form
        one = D * 8
        for f, fd, nin in ((dec, decd, count), (rec, recd, count * k)):
            for off in (0, one, 8, one * (nin - 1), -one):
                assert f(ctx, px, count, b, k, 0, at(x.ctypes.data + off)) == E_ARG and "overlaps" in err(ctx), off
            assert fd(ctx, x.ctypes.data, count, b, k, 1, x.ctypes.data + one) == E_ARG and "overlaps" in err(ctx)
        assert np.array_equal(x, ref.rand_ring(0xA1, (count * k, D))) and (out == SENT).all() and am.value == SENT
        # the context is usable
        assert np.array_equal(ctx.balanced_recompose(ctx.balanced_decompose(x[:count], 2**62, 2), 2**62, 2), x[:count])
    finally:
        sharded.close()


def test_device_pointer_refusals(ctx):
    count, b, k = 24, 3, 2
    x = ref.rand_ring(0xA2, (count, D))
    xv, xw = dev_view(x)
    ov, ow = dev_view(np.full((count * k, D), SENT, dtype=np.uint64))
    torch.cuda.empty_cache()
    big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")      # an allocation of its own (requested from an empty cache)
    pinned = torch.zeros((count * k, D), dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    pageable = np.zeros((count * k, D), dtype=np.uint64)
    am = C.c_uint64(SENT)
    good = (xv.data_ptr(), ov.data_ptr())
    bad = [("pinned host memory", lambda slot: pinned.data_ptr()), ("pageable host memory", lambda slot: pageable.ctypes.data), ("dev + 8", lambda slot: good[slot] + 8),
           ("off the end", lambda slot: big.data_ptr() + (32 << 20) - 128)]
    for name, addr in bad:
        for slot in range(2):
            args = list(good)
            args[slot] = addr(slot)
            assert decd(ctx, args[0], count, b, k, 0, args[1]) == E_ARG and "device memory" in err(ctx), (name, slot)
            assert recd(ctx, args[1], count, b, k, 0, args[0]) == E_ARG and "device memory" in err(ctx), (name, slot)
        assert L().lfplus_linf_norm_device(ctx.h, addr(0), count, C.byref(am)) == E_ARG and "device memory" in err(ctx), name
    assert (host(ov) == SENT).all() and np.array_equal(host(xv), x) and am.value == SENT and margins_intact(ow) and margins_intact(xw)
    # the same arrays, well-formed
    assert decd(ctx, good[0], count, b, k, 0, good[1]) == 0 and np.array_equal(host(ov), dref.decompose(x, b, k, GADGET))
    assert L().lfplus_linf_norm_device(ctx.h, good[0], count, C.byref(am)) == 0 and am.value == dref.linf(x)


@pytest.mark.parametrize("word", [P, 2**64 - 1])
def test_non_canonical_words(ctx, word):
    """found by the kernel that reads the word: a host out stays untouched, the flag is home before the call returns"""
    count, b, k = 19, 10**9 + 7, 3
    x = ref.rand_ring(0xA3, (count * k, D))
    am = C.c_uint64(SENT)
    for f, fd, nin, nout in ((dec, decd, count, count * k), (rec, recd, count * k, count)):
        for where in ((0, 0), (nin - 1, D - 1)):
            y = x[:nin].copy()
            y[where] = word
            out = np.full((nout, D), SENT, dtype=np.uint64)
            for layout in (0, 1):
                assert f(ctx, hp(y), count, b, k, layout, hp(out)) == E_ARG and "non-canonical" in err(ctx), (where, layout)
                assert (out == SENT).all()
            yv, yw = dev_view(y)
            ov, ow = dev_view(out)
            assert fd(ctx, yv.data_ptr(), count, b, k, 0, ov.data_ptr()) == E_ARG and "non-canonical" in err(ctx)
            assert margins_intact(ow) and np.array_equal(host(yv), y)
            if nin == count:
                assert L().lfplus_linf_norm(ctx.h, hp(y), count, C.byref(am)) == E_ARG and "non-canonical" in err(ctx) and am.value == SENT
                assert L().lfplus_linf_norm_device(ctx.h, yv.data_ptr(), count, C.byref(am)) == E_ARG and "non-canonical" in err(ctx) and am.value == SENT
    assert np.array_equal(ctx.balanced_decompose(x[:count], b, k), dref.decompose(x[:count], b, k, GADGET)), "the context is usable"


def smg(c, rows, m, b, k, n, mats, nM=None):
    keep, rp, cp, vp = plus._csr_args(mats)
    return L().lfplus_set_matrices_gadget(c.h, rows, m, b, k, n, len(mats) if nM is None else nM, rp, cp, vp)


def test_refusals_of_set_matrices_gadget_leave_the_resident_matrices():
    n, m, k, b = 64, 16, 4, 3
    resident = [ref.rand_csr(0xB0 + q, n, 2) for q in range(2)]
    short = [_ragged(0xB4 + q, m, m, const=False) for q in range(3)]
    x = ref.rand_ring(0xB8, (n, D))
    c, sharded = plus.PlusContext(0), plus.PlusContext(0)
    try:
        sharded.set_sharding_model(0, 2)
        c.set_matrices(resident, n=n)
        want = [c.spmv(j, x) for j in range(2)] + [c.spmv_t(j, x) for j in range(2)]

        def intact():
            return all(np.array_equal(a, w) for a, w in zip([c.spmv(j, x) for j in range(2)] + [c.spmv_t(j, x) for j in range(2)], want))
        # a NULL array
        assert L().lfplus_set_matrices_gadget(c.h, m, m, b, k, n, 3, None, None, None) == E_ARG and "null" in err(c) and intact()
        # the envelope, before the sharded context
        for cc in (c, sharded):
            for rows_, m_, b_, k_, n_, nM_ in ((m, m, b, k, n + 1, 3), (n + 1, m, b, k, n, 3), (m, m, b, 0, n, 3), (m, 1, b, 65, 65, 3), (m, m, 1, k, n, 3),
                                               (m, m, 2**62 + 1, k, n, 3), (m, m, b, k, 0, 3), (m, m + 1, b, k, n, 3), (m, m, b, k, n, 65)):
                assert smg(cc, rows_, m_, b_, k_, n_, short, nM_) == E_ARG and "envelope" in err(cc), (rows_, m_, b_, k_, n_, nM_)
        assert intact()
        assert smg(sharded, m, m, b, k, n, short) == E_ARG and "sharded" in err(sharded)
        # the CSR arrays, as lfplus_set_matrices validates them; a bad LAST matrix: the first two were already expanded and are dropped again
        for what, edit in (("malformed", lambda rp, col, val: rp.__setitem__(0, 1)), ("monotone", lambda rp, col, val: rp.__setitem__(3, int(rp[-1]) + 1)),
                           ("column", lambda rp, col, val: col.__setitem__(col.size - 1, m)), ("non-canonical", lambda rp, col, val: val.__setitem__((0, 15), P))):
            bad = [tuple(a.copy() for a in mat) for mat in short]
            edit(*bad[2])
            assert smg(c, m, m, b, k, n, bad) == E_ARG and what in err(c), what
            assert intact(), what
        # the same arrays, well-formed, replace the set; nM == 0 drops it
        c.set_matrices_gadget(short, m, b, k)
        twin = plus.PlusContext(0)
        try:
            twin.set_matrices(plus.r1cs_decomposed_square(short, n, b, k), n=n)
            assert all(np.array_equal(c.spmv(j, x), twin.spmv(j, x)) and np.array_equal(c.spmv_t(j, x), twin.spmv_t(j, x)) for j in range(3))
        finally:
            twin.close()
        assert smg(c, m, m, b, k, n, [], 0) == 0
        y = np.full((n, D), SENT, dtype=np.uint64)
        assert L().lfplus_spmv(c.h, 0, hp(x), n, hp(y)) == E_ARG and "no resident matrices" in err(c)
    finally:
        c.close()
        sharded.close()
