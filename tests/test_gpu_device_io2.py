"""Device-memory twins of the component calls: lf_decompose_dev, lf_recompose_dev, lf_linf_check_dev, lf_build_eq_dev, lf_mle_eval_batch_dev, lf_spmv_dev,
lf_sumcheck_{lin,fold}_begin_dev, lf_lincomb_dev, lf_horner_combine_dev.  The yardstick is the host-pointer twin on the same context (itself tested against the
oracle); decompose, spmv, mle_eval and one linearization sumcheck are compared with the oracle directly as well.  Every comparison is exact equality of words.

Shapes: counts 1, 63, 65, 333 around the 64-element tile of the relayout block; nv 1, 5, 6, 7 around the threshold of the two-level eq build; T8 / B6 (m = 256 /
64) for the calls that need a constraint system.  No table here has more than 2^10 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_corners as fc
from latticefold_amd import api
from latticefold_amd.workload import RINGS, diag, make_workload, splitmix_fq
from test_gpu_ext_basis import random_T, tower_T

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, STATE = -1, -3, -7
COUNTS = (1, 63, 65, 333)
SENTINEL = np.uint64(2**64 - 1)
NAMES = {"goldilocks": "T8", "babybear": "B6"}


def _oracle(ring):
    if ring == "goldilocks":
        import lfo as O
    else:
        import lfo_bb as O
    return O


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def blank(*shape):
    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


def untouched(t):
    return bool((host(t) == SENTINEL).all())


def _rnd(seed, ring, *shape):
    return splitmix_fq(seed, 0, int(np.prod(shape)), ring).reshape(shape).copy()


def _embed(ch):
    return np.tile(np.asarray(ch, dtype=np.uint64), 8)


@pytest.fixture(scope="module", params=["goldilocks", "babybear"])
def rc(request):
    """(ring, context with T8 / B6 loaded, workload)"""
    ring = request.param
    wl = make_workload(NAMES[ring])
    ctx = api.Context(0, ring=ring)
    ctx.load_ccs(wl)
    yield ring, ctx, wl
    ctx.close()


# ---- 1. parity with the host twin (and the oracle) -------------------------------------------------------------------------------------------------------------
def _bases(ring):
    """(base, digits, values small enough for the digits?)"""
    return ((2, 16, True), (1 << 16, 4 if ring == "goldilocks" else 2, False)) + (((1 << 63, 2, False),) if ring == "goldilocks" else ())


@pytest.mark.parametrize("count", COUNTS)
def test_decompose_recompose(rc, count):
    ring, ctx, _wl = rc
    O, p = _oracle(ring), RINGS[ring][0]
    x = _rnd(3 + count, ring, count, ctx.RE)
    x[0, :6] = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2, 2**15]
    for base, digits, small in _bases(ring):
        src = O.decompose(x, 1 << 16, 4, 0)[:count] if small else x      # base 2: 16-bit digits as values
        for layout in (0, 1):
            want = ctx.decompose(src, base, digits, layout)
            if base != 1 << 63:
                assert (want == O.decompose(src, base, digits, layout)).all(), (base, layout, "host twin against the oracle")
            sd = dev(src)
            got = ctx.decompose(sd, base, digits, layout)
            assert (host(got) == want).all(), (ring, count, base, layout)
            assert (host(sd) == src).all(), "the input was written"
            o = blank(count * digits, ctx.RE)
            assert ctx.decompose(sd, base, digits, layout, out=o) is o and (host(o) == want).all()
        d = ctx.decompose(src, base, digits, 0)
        want = ctx.recompose(d, base, digits)
        assert (host(ctx.recompose(dev(d), base, digits)) == want).all(), (ring, count, base, "recompose")
        if base != 1 << 63:
            assert (want == src).all()


def test_linf_check_with_the_maximum_in_the_last_element(rc):
    ring, ctx, _wl = rc
    O, p = _oracle(ring), RINGS[ring][0]
    c = np.zeros((65, ctx.RE), dtype=np.uint64)
    c[3, 5] = 70
    c[64, ctx.RE - 1] = p - 123
    f = O.crt(c)
    fd = dev(f)
    for bound, unsigned in ((124, False), (123, False), (1 << 20, True), (p, True)):
        want = ctx.linf_check(f, bound, unsigned_variant=unsigned)
        assert ctx.linf_check(fd, bound, unsigned_variant=unsigned) == want, (ring, bound, unsigned)
    assert ctx.linf_check(fd, 124) == (True, 123) and ctx.linf_check(fd, 123)[0] is False
    assert ctx.linf_check(fd, 1 << 20, unsigned_variant=True) == (False, p - 123)


@pytest.mark.parametrize("nv", [1, 5, 6, 7])      # the two-level build starts at 6
def test_build_eq_into_device_memory(rc, nv):
    ring, ctx, _wl = rc
    pt = _rnd(40 + nv, ring, nv, ctx.TAU)
    want = ctx.build_eq(pt)
    o = blank(1 << nv, ctx.TAU)
    assert ctx.build_eq(pt, out=o) is o
    assert (host(o) == want).all(), (ring, nv)


@pytest.mark.parametrize("ntables,ln,nv", [(1, 64, 6), (5, 65, 7), (3, 13, 4)])
def test_mle_eval_batch(rc, ntables, ln, nv):
    ring, ctx, _wl = rc
    O = _oracle(ring)
    pt = _rnd(50 + nv, ring, nv, ctx.TAU)
    tabs = _rnd(60 + ln, ring, ntables, ln, ctx.RE)
    want = ctx.evaluate_mles(tabs, pt)
    ring_pt = np.stack([_embed(c) for c in pt])
    for a in range(ntables):
        assert (want[a] == O.mle_eval(tabs[a], ring_pt)).all(), "host twin against the oracle"
    td = dev(tabs)
    assert (ctx.evaluate_mles(td, pt) == want).all(), (ring, ntables, ln, nv)
    assert (host(td) == tabs).all()


def _spmv_by_rows(O, wl, j, z):
    """M_j z of a matrix with at most one entry per row, through the oracle's ring product"""
    rp, ci = np.asarray(wl.rowptr[j]).astype(np.int64), np.asarray(wl.col[j]).astype(np.int64)
    assert (np.diff(rp) <= 1).all()
    rows = np.nonzero(np.diff(rp))[0]
    val = np.ascontiguousarray(np.asarray(wl.val[j], dtype=np.uint64).reshape(-1, wl.RE))
    zz = np.ascontiguousarray(z[ci])
    prod = np.zeros((rows.size, wl.RE), dtype=np.uint64)
    O.lib().lfo_ring_mul_ntt(O._p64(val), O._p64(zz), O._p64(prod), rows.size)
    out = np.zeros((wl.m, wl.RE), dtype=np.uint64)
    out[rows] = prod
    return out


@pytest.mark.parametrize("name,ccs", [("T8", "r1cs"), ("T8", "multi"), ("B6", "r1cs"), ("B6", "deg3")])
def test_spmv(name, ccs):
    wl = make_workload(name, ccs=ccs)
    O = _oracle(wl.ring)
    if (name, ccs) == ("T8", "multi"):     # the general CSR rows: k_spmv_rows gathers whole elements from the caller's z itself
        assert int(wl.rowptr[0][-1]) * 2 > min(wl.n, wl.m) * 3
    ctx = api.Context(0, ring=wl.ring)
    try:
        ctx.load_ccs(wl)
        z = wl.z()
        zd = dev(z)
        o = blank(wl.m, ctx.RE)
        for j in range(wl.t):
            want = ctx.mat_vec_mul(j, z)
            if ccs == "r1cs":
                assert (want == _spmv_by_rows(O, wl, j, z)).all(), "host twin against the oracle"
            assert (host(ctx.mat_vec_mul(j, zd)) == want).all(), (name, ccs, j)
            assert ctx.mat_vec_mul(j, zd, out=o) is o and (host(o) == want).all()
        assert (host(zd) == z).all()
    finally:
        ctx.close()


def _challenges(ring, s, tau):
    return _rnd(91, ring, s, tau)


def _lin_messages(ctx, wl, tables, beta, ch):
    sc = api.MLSumcheckLin(ctx, tables, beta)
    msgs = [sc.prove_round(None if r == 0 else ch[r - 1]) for r in range(wl.s)]
    with pytest.raises(api.LfError):
        sc.prove_round(ch[-1])                       # "Prover is not active"
    sc.end()
    return np.stack(msgs)


def _fold_tables(wl, O):
    m, tau, K2 = wl.m, wl.tau, 2 * wl.K
    nt = 5 + K2 * tau
    tables = _rnd(77, wl.ring, nt, m, wl.RE)
    for idx, sd in ((0, 1), (2, 2), (4, 3)):         # the three eq tables are slot-constant: real eq tables of random points
        pt = _rnd(100 + sd, wl.ring, wl.s, tau)
        tables[idx] = O.build_eq(np.stack([_embed(c) for c in pt]))
    mu = _rnd(9, wl.ring, K2, tau)
    mu[-1] = 0
    mu[-1, 0] = 1
    return tables, mu


def _fold_messages(ctx, wl, tables, mu, ch):
    sc = api.MLSumcheckFold(ctx, tables, mu)
    msgs = [sc.prove_round(None if r == 0 else ch[r - 1]) for r in range(wl.s)]
    sc.end()
    return np.stack(msgs)


@pytest.mark.parametrize("name,ccs", [("T8", "r1cs"), ("B6", "r1cs"), ("T8", "deg5")])
def test_sumchecks_begun_from_device_tables(name, ccs):
    wl = make_workload(name, ccs=ccs)
    O = _oracle(wl.ring)
    ctx = api.Context(0, ring=wl.ring)
    try:
        ctx.load_ccs(wl)
        ch = _challenges(wl.ring, wl.s, wl.tau)
        tables = _rnd(70 + wl.t, wl.ring, wl.t, wl.m, wl.RE)
        beta = _rnd(71, wl.ring, wl.s, wl.tau)
        want = _lin_messages(ctx, wl, tables, beta, ch)
        td = dev(tables)
        assert (_lin_messages(ctx, wl, td, beta, ch) == want).all(), (name, ccs, "lin")
        assert (host(td) == tables).all()
        ftab, mu = _fold_tables(wl, O)
        want = _fold_messages(ctx, wl, ftab, mu, ch)
        fd = dev(ftab)
        assert (_fold_messages(ctx, wl, fd, mu, ch) == want).all(), (name, ccs, "fold")
        # an eq table that is not slot-constant is refused on the device as it is on the host, and nothing is begun
        bad = ftab.copy()
        bad[4, wl.m - 1, wl.RE - 1] ^= np.uint64(1)
        for arg in (bad, dev(bad)):
            with pytest.raises(api.LfError) as e:
                api.MLSumcheckFold(ctx, arg, mu)
            assert e.value.code == UNSUPPORTED
        assert (_fold_messages(ctx, wl, fd, mu, ch) == want).all()
    finally:
        ctx.close()


def test_linearization_sumcheck_from_device_tables_against_the_oracle():
    """lf_sumcheck_lin_begin_dev on the tables M_j z that lf_spmv_dev left on the device, driven by a replay of the Fiat-Shamir schedule: every round message is the
    oracle's LinearizationProof"""
    import lfo
    wl = make_workload("T8")
    p, RE = RINGS["goldilocks"][0], 24
    inst = lfo.Instance(wl)
    ctx = api.Context(0)
    try:
        ctx.load_ccs(wl)
        A = wl.ajtai_matrix()
        f_coeff = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([lfo.ajtai_commit(A, wl.kappa, wl.N, lfo.crt(f_coeff)), wl.x_ccs])
        lc_o, pr_o = inst.linearize(lfo.Transcript(), cccs, f_coeff)
        tr = api.PoseidonTranscript()
        tr.absorb_slice(diag(int.from_bytes(b"beta_s", "big") % p)[None, :])
        beta = np.stack([tr.get_challenge() for _ in range(wl.s)])
        tables = blank(wl.t, wl.m, RE)
        zd = dev(wl.z())
        for j in range(wl.t):
            ctx.mat_vec_mul(j, zd, out=tables[j])
        sc = api.MLSumcheckLin(ctx, tables, beta)
        tr.absorb_slice(diag(wl.s)[None, :])
        tr.absorb_slice(diag(wl.d + 1)[None, :])
        npts, r = wl.d + 2, None
        for rnd in range(wl.s):
            msg = sc.prove_round(r)
            assert (msg == pr_o[rnd * npts:(rnd + 1) * npts]).all(), rnd
            tr.absorb_slice(msg)
            r = tr.get_challenge()
            tr.absorb_slice(_embed(r)[None, :])
            assert (_embed(r) == lc_o[rnd]).all()
        sc.end()
    finally:
        ctx.close()


@pytest.mark.parametrize("K,ln", fc.COMBINE_CASES)
def test_lincomb_and_horner_combine(rc, K, ln):
    ring, ctx, _wl = rc
    coef, tabs = fc.lincomb_case(K, ln, ring)
    want = api.lincomb(ctx, coef, tabs)
    td = dev(tabs)
    assert (host(api.lincomb(ctx, coef, td)) == want).all(), (ring, K, "lincomb")
    o = blank(ln, ctx.RE)
    assert api.lincomb(ctx, coef, td, out=o) is o and (host(o) == want).all() and (host(td) == tabs).all()
    tabs, ch = fc.horner_case(K, ln, ring)
    want = api.horner_combine(ctx, tabs, ch)
    td = dev(tabs)
    assert (host(api.horner_combine(ctx, td, ch)) == want).all(), (ring, K, "horner_combine")
    o = blank(ln, ctx.RE)
    assert api.horner_combine(ctx, td, ch, out=o) is o and (host(o) == want).all()


# ---- 2. external basis: NTT-form arrays change basis in the relayout pass, coefficient-form arrays do not -------------------------------------------------------
@pytest.mark.parametrize("ring,kind", [("babybear", "tower"), ("goldilocks", "random")])
def test_dev_calls_in_an_external_basis(ring, kind):
    T = tower_T() if kind == "tower" else random_T(ring, 4242)
    wl = make_workload(NAMES[ring])
    ctx = api.Context(0, ring=ring)
    try:
        ctx.set_ext_basis(T)
        ctx.load_ccs(wl)
        RE, tau = ctx.RE, ctx.TAU
        plain = api.Context(0, ring=ring)
        try:       # (the basis does change the words: the comparison below is not vacuous)
            pt = _rnd(1, ring, 6, tau)
            assert not (plain.build_eq(pt) == ctx.build_eq(pt)).all()
        finally:
            plain.close()
        pt = _rnd(1, ring, 7, tau)
        tabs = _rnd(2, ring, 3, 65, RE)
        assert (ctx.evaluate_mles(dev(tabs), pt) == ctx.evaluate_mles(tabs, pt)).all(), "mle_eval_batch"
        z = _rnd(3, ring, wl.n, RE)
        for j in range(wl.t):
            assert (host(ctx.mat_vec_mul(j, dev(z))) == ctx.mat_vec_mul(j, z)).all(), ("spmv", j)
        if ring == "goldilocks":      # general CSR rows in an external basis: the element-major copy is rebuilt from the converted planes, not the caller's z
            wm = make_workload("T8", ccs="multi")
            assert int(wm.rowptr[0][-1]) * 2 > min(wm.n, wm.m) * 3
            ctx.load_ccs(wm)
            zm = _rnd(13, ring, wm.n, RE)
            for j in range(wm.t):
                assert (host(ctx.mat_vec_mul(j, dev(zm))) == ctx.mat_vec_mul(j, zm)).all(), ("spmv, general rows", j)
        coef, t2 = _rnd(4, ring, 3, RE), _rnd(5, ring, 3, 65, RE)
        assert (host(api.lincomb(ctx, coef, dev(t2))) == api.lincomb(ctx, coef, t2)).all(), "lincomb"
        x = _rnd(6, ring, 65, RE)
        want = ctx.decompose(x, 1 << 16, 2, 1)
        assert (want == _oracle(ring).decompose(x, 1 << 16, 2, 1)).all(), "coefficient form has no basis"
        assert (host(ctx.decompose(dev(x), 1 << 16, 2, 1)) == want).all(), "decompose"
        for nv in (5, 6):
            pt = _rnd(7 + nv, ring, nv, tau)
            assert (host(ctx.build_eq(pt, out=blank(1 << nv, tau))) == ctx.build_eq(pt)).all(), ("build_eq", nv)
    finally:
        ctx.close()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def _hip():
    """the HIP runtime this process has loaded already (one allocation of an exact size: what the caching allocator of torch never hands out)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            lib.hipFree.argtypes = [C.c_void_p]
            return lib
    raise RuntimeError("no HIP runtime loaded")


class Calls:
    """the ten calls on one context at small fixed shapes: name -> (call(pointers), {argument: bytes}, inputs, output or None)"""

    def __init__(self, ctx, wl):
        L, h, RE, tau = api._lib(), ctx.h, ctx.RE, ctx.TAU
        self.RE, e = RE, RE * 8
        n, m, nf = wl.n, wl.m, 5 + 2 * wl.K * tau
        self.ok, self.mx = C.c_int(77), C.c_uint64(77)
        self.pt = np.ascontiguousarray(_rnd(1, wl.ring, 8, tau))
        self.mu = np.ascontiguousarray(_rnd(2, wl.ring, 2 * wl.K, tau))
        self.coef = np.ascontiguousarray(_rnd(3, wl.ring, 2, RE))
        self.ev = np.full((2, RE), SENTINEL, dtype=np.uint64)
        u = lambda a: a.ctypes.data_as(api.u64p)
        pt, mu, coef, ev = u(self.pt), u(self.mu), u(self.coef), u(self.ev)
        B = 1 << 16
        self.table = {
            "decompose": (lambda a: L.lf_decompose_dev(h, a["in"], 65, B, 2, 1, a["out"]), {"in": 65 * e, "out": 130 * e}),
            "recompose": (lambda a: L.lf_recompose_dev(h, a["in"], 65, B, 2, a["out"]), {"in": 130 * e, "out": 65 * e}),
            "linf_check": (lambda a: L.lf_linf_check_dev(h, a["in"], 65, 1000, 0, C.byref(self.ok), C.cast(C.byref(self.mx), api.u64p)), {"in": 65 * e}),
            "build_eq": (lambda a: L.lf_build_eq_dev(h, pt, 6, a["out"]), {"out": 64 * tau * 8}),
            "mle_eval_batch": (lambda a: L.lf_mle_eval_batch_dev(h, a["in"], 2, 65, pt, 7, ev), {"in": 130 * e}),
            "spmv": (lambda a: L.lf_spmv_dev(h, 0, a["in"], a["out"]), {"in": n * e, "out": m * e}),
            "sumcheck_lin_begin": (lambda a: L.lf_sumcheck_lin_begin_dev(h, a["in"], pt), {"in": wl.t * m * e}),
            "sumcheck_fold_begin": (lambda a: L.lf_sumcheck_fold_begin_dev(h, a["in"], mu), {"in": nf * m * e}),
            "lincomb": (lambda a: L.lf_lincomb_dev(h, coef, a["in"], 2, 65, a["out"]), {"in": 130 * e, "out": 65 * e}),
            "horner_combine": (lambda a: L.lf_horner_combine_dev(h, a["in"], 2, 1, 65, pt, a["out"]), {"in": 130 * e, "out": 65 * e}),
        }
        self.no_overlap = ("decompose", "recompose", "spmv", "lincomb", "horner_combine")

    def good(self, name, seed=0, ring=None):
        """fresh device arrays of a call: canonical input (zeros, or pseudo-random words), a sentinel-filled output"""
        sizes = self.table[name][1]
        bufs = {}
        if "in" in sizes:
            w = sizes["in"] // 8
            bufs["in"] = dev(_rnd(seed, ring, w)) if ring else torch.zeros(w, dtype=torch.int64, device="cuda")
        if "out" in sizes:
            bufs["out"] = blank(sizes["out"] // 8)
        return bufs

    def run(self, name, bufs, **override):
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        ptrs.update(override)
        return self.table[name][0](ptrs)

    def host_side_untouched(self):
        return (self.ok.value, self.mx.value) == (77, 77) and bool((self.ev == SENTINEL).all())

    def reset_host_side(self):
        self.ok.value, self.mx.value = 77, 77
        self.ev[:] = SENTINEL


def _round_code(ctx, which):
    """the code of a first round of the `which` sumcheck (a success advances it)"""
    o = np.zeros((9, ctx.RE), dtype=np.uint64)
    return getattr(api._lib(), f"lf_sumcheck_{which}_round")(ctx.h, None, o.ctypes.data_as(api.u64p))


def _end_both(ctx):
    assert api._lib().lf_sumcheck_lin_end(ctx.h) == 0 and api._lib().lf_sumcheck_fold_end(ctx.h) == 0


def test_bad_pointers_and_overlaps_are_refused(rc):
    ring, ctx, wl = rc
    calls = Calls(ctx, wl)
    hip = _hip()
    raw = []
    _end_both(ctx)
    try:
        for name, (_fn, sizes) in calls.table.items():
            bufs = calls.good(name)
            for arg, nbytes in sizes.items():
                elem = ctx.TAU * 8 if name == "build_eq" else ctx.RE * 8
                host_arr = np.zeros(nbytes // 8, dtype=np.uint64)
                pinned = torch.zeros(nbytes // 8, dtype=torch.int64).pin_memory()
                short = C.c_void_p()
                assert hip.hipMalloc(C.byref(short), nbytes - elem) == 0        # one element short of the range the call touches
                raw.append(short)
                bad = {"numpy": host_arr.ctypes.data, "pinned": pinned.data_ptr(), "misaligned": bufs[arg].data_ptr() + 4, "short": short.value}
                for why, q in bad.items():
                    assert calls.run(name, bufs, **{arg: q}) == INVALID, (ring, name, arg, why)
                assert not host_arr.any() and not pinned.numpy().any()
            if name in calls.no_overlap:      # out starts one element into the input, and the input one element into out
                big = torch.zeros((sizes["in"] + sizes["out"]) // 8, dtype=torch.int64, device="cuda")
                p0 = big.data_ptr()
                assert calls.run(name, {}, **{"in": p0, "out": p0 + ctx.RE * 8}) == INVALID, (ring, name, "overlap")
                assert calls.run(name, {}, **{"in": p0 + ctx.RE * 8, "out": p0}) == INVALID, (ring, name, "overlap")
                assert calls.run(name, {}, **{"in": p0, "out": p0 + sizes["in"]}) == 0, (ring, name, "disjoint halves of one allocation")
            if "out" in bufs:
                assert untouched(bufs["out"]), (ring, name)
            assert calls.host_side_untouched(), (ring, name)
        assert (_round_code(ctx, "lin"), _round_code(ctx, "fold")) == (STATE, STATE)       # no refused begin began anything
    finally:
        for q in raw:
            hip.hipFree(q)
    # the context goes on working
    x = _rnd(8, ring, 65, ctx.RE)
    assert (host(ctx.decompose(dev(x), 1 << 16, 2, 1)) == ctx.decompose(x, 1 << 16, 2, 1)).all()
    z = wl.z()
    assert (host(ctx.mat_vec_mul(0, dev(z))) == ctx.mat_vec_mul(0, z)).all()


def test_non_canonical_words_are_refused_by_the_device(rc):
    ring, ctx, wl = rc
    p = RINGS[ring][0]
    calls = Calls(ctx, wl)
    words = (p,) + ((2**64 - 1,) if ring == "babybear" else ())
    _end_both(ctx)
    for name, (_fn, sizes) in calls.table.items():
        if "in" not in sizes:
            continue                                   # lf_build_eq_dev has no device input
        n_in = sizes["in"] // 8
        calls.reset_host_side()
        for word in words:
            for pos in (0, n_in - 1):                  # the first word of the first table, the last word of the last one
                bufs = calls.good(name)
                bufs["in"][pos] = np.array(word, dtype=np.uint64).view(np.int64).item()
                assert calls.run(name, bufs) == INVALID, (ring, name, word, pos)
                if "out" in bufs:
                    assert untouched(bufs["out"]), (ring, name, word, pos)
                assert calls.host_side_untouched(), (ring, name)
                if name.startswith("sumcheck"):
                    assert _round_code(ctx, name.split("_")[1]) == STATE
        bufs = calls.good(name)                         # the same call with clean input
        assert calls.run(name, bufs) == 0, (ring, name)
        if "out" in bufs:
            assert not untouched(bufs["out"])
    assert (_round_code(ctx, "lin"), _round_code(ctx, "fold")) == (0, 0)                  # both clean begins began
    _end_both(ctx)
    # a failed begin ends a sumcheck that was in progress: its tables are gone
    bufs = calls.good("sumcheck_lin_begin")
    assert calls.run("sumcheck_lin_begin", bufs) == 0
    bufs["in"][-1] = np.array(p, dtype=np.uint64).view(np.int64).item()
    assert calls.run("sumcheck_lin_begin", bufs) == INVALID and _round_code(ctx, "lin") == STATE


def test_state_and_envelope_codes_come_before_the_pointer_checks():
    for ring in ("goldilocks", "babybear"):
        ctx = api.Context(0, ring=ring)
        try:
            L, RE = api._lib(), ctx.RE
            hbuf = np.zeros((400, RE), dtype=np.uint64)       # a HOST pointer: it is never looked at
            q = hbuf.ctypes.data
            pt = hbuf.ctypes.data_as(api.u64p)
            assert L.lf_decompose_dev(ctx.h, q, 65, 6, 2, 0, q) == UNSUPPORTED
            assert L.lf_decompose(ctx.h, pt, 65, 6, 2, 0, pt) == UNSUPPORTED
            assert L.lf_spmv_dev(ctx.h, 0, q, q) == STATE and L.lf_spmv(ctx.h, 0, pt, pt) == STATE
            assert L.lf_sumcheck_lin_begin_dev(ctx.h, q, pt) == STATE and L.lf_sumcheck_lin_begin(ctx.h, pt, pt) == STATE
            assert L.lf_sumcheck_fold_begin_dev(ctx.h, q, pt) == STATE and L.lf_sumcheck_fold_begin(ctx.h, pt, pt) == STATE
            assert L.lf_mle_eval_batch_dev(ctx.h, q, 1, 65, pt, 6, pt) == INVALID       # IncorrectLength: 65 > 2^6
            ctx.load_ccs(make_workload(NAMES[ring]))
            assert L.lf_spmv_dev(ctx.h, 99, q, q) == INVALID                           # no such matrix
            assert L.lf_spmv_dev(ctx.h, 0, q, q) == INVALID                            # now the pointer is looked at
            assert not hbuf.any()
        finally:
            ctx.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_tables_produced_on_another_torch_stream(rc):
    """the tables are still being written by kernels of a side stream when the call is made: lf_ctx_wait_stream orders the context behind that stream, nobody
    synchronises it.  A chain of 4096 x 4096 products is queued on the side stream ahead of the copy that produces the tables (tens of milliseconds of work,
    and the copy reads a buffer the chain's last product seeds), so the tables do not exist yet when the library is called: until they do the buffer holds the
    sentinel, which is not canonical, and a call that did not wait would be refused"""
    ring, ctx, _wl = rc
    L = api._lib()
    ln, nv = 333, 9
    tabs = _rnd(77, ring, 2, ln, ctx.RE)
    pt = _rnd(78, ring, nv, ctx.TAU)
    want = ctx.evaluate_mles(tabs, pt)
    base = dev(tabs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = np.zeros((2, ctx.RE), dtype=np.uint64)
    t = blank(2, ln, ctx.RE)
    a = torch.full((4096, 4096), 1.0 / 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(24):
            a = a @ a                                    # (every entry stays 1 / 4096)
        t.copy_(base + (a[0, 0] * 0).to(torch.int64))    # the tables depend on the chain's last product
        ctx.wait_stream(side.cuda_stream)
        assert L.lf_mle_eval_batch_dev(ctx.h, t.data_ptr(), 2, ln, pt.ctypes.data_as(api.u64p), nv, got.ctypes.data_as(api.u64p)) == 0
    assert (got == want).all()
    assert (ctx.evaluate_mles(t, pt) == want).all()      # (and synchronised)
