"""lf_ring_mul / lf_ring_mul_device: sums of products of arrays of ring elements, in NTT form and in coefficient form, on both rings.

Every reference is independent of the code under test: the numpy schoolbook of latticefold_amd.workload (ring_mul_ntt, _fp_add) for NTT-form products, Python
integers in F_p[Y]/(Y^tau - nu) (field_corners.Ref) at the reduction corners, and for coefficient-form products the big-integer schoolbook product reduced by
X^k = X^(k - d/2) - X^(k - d) and then mod p.  Every comparison is exact equality of words.

Shapes: counts 1, 67, 259, 4099 leave relayout tiles (64 elements), the one-wave blocks of the fused kernel (64) and the 256-thread blocks of the slot kernel half
empty; 1, 2, 9, 33 terms take the single-product tail, one pair, pairs and a tail, and more terms than any power-of-two flush interval up to 32."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_corners as fc
from latticefold_amd import api
from latticefold_amd.workload import RINGS, _fp_add, diag, make_workload, ring_mul_ntt, splitmix_fq
from ring_mul_refs import coeff_sum_bigint, ntt_sum_bigint, ntt_sum_numpy
from test_gpu_device_io2 import _hip
from test_gpu_ext_basis import _inv_matrix, random_T, tower_T
from test_gpu_ext_basis_device import slotwise

pytestmark = pytest.mark.gpu
INVALID = -1
SENTINEL = np.uint64(2**64 - 1)
NAMES = {"goldilocks": "T8", "babybear": "B6"}
FORM = api.FORMS


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


@pytest.fixture(scope="module", params=["goldilocks", "babybear"])
def rc(request):
    """(ring, a BARE context: no constraint system, no matrix)"""
    ring = request.param
    ctx = api.Context(0, ring=ring)
    yield ring, ctx
    ctx.close()


# ---- 1. NTT form against numpy ---------------------------------------------------------------------------------------------------------------------------------------
TERMS = (1, 2, 9, 33)


@pytest.fixture(scope="module")
def ntt_operands():
    """per ring: (a, b) of 33 x 4099 elements, made once; a case takes the leading terms and elements"""
    return {ring: (_rnd(101, ring, 33, 4099, RINGS[ring][1]), _rnd(102, ring, 33, 4099, RINGS[ring][1])) for ring in RINGS}


@pytest.mark.parametrize("count", [1, 67, 259, 4099])
def test_ntt_form_against_numpy(rc, ntt_operands, count):
    ring, ctx = rc
    a, b = (np.ascontiguousarray(v[:, :count]) for v in ntt_operands[ring])
    want = np.zeros((count, ctx.RE), dtype=np.uint64)
    done = 0
    for nt in TERMS:                                   # the expected sums grow term by term: every product is formed once
        want = _fp_add(want, ntt_sum_numpy(a[done:nt], b[done:nt], ring), ring)
        done = nt
        got = ctx.ring_mul(a[:nt], b[:nt])
        assert got.shape == (count, ctx.RE) and (got == want).all(), (ring, count, nt)
    assert (ctx.ring_mul(a[0], b[0]) == ring_mul_ntt(a[0], b[0], ring)).all()      # the (count, RE) spelling of one term


# ---- 2. coefficient form against big integers ------------------------------------------------------------------------------------------------------------------------
def _through_ntt(ctx, a, b):
    return ctx.ntt_inv(ctx.ring_mul(ctx.ntt_fwd(a), ctx.ntt_fwd(b)))


@pytest.mark.parametrize("count,nt", [(1, 1), (67, 1), (259, 1), (1, 3), (67, 3), (259, 3)])
def test_coefficient_form_against_big_integers(rc, count, nt):
    ring, ctx = rc
    a, b = _rnd(201 + count, ring, nt, count, ctx.RE), _rnd(202 + count, ring, nt, count, ctx.RE)
    got = ctx.ring_mul(a, b, form="coeff")
    assert (got == coeff_sum_bigint(a, b, ring)).all(), (ring, count, nt)
    assert (got == _through_ntt(ctx, a, b)).all(), "the fused product is the product of the transforms, transformed back"


def test_coefficient_form_at_4099_elements_through_the_transforms(rc):
    ring, ctx = rc
    a, b = _rnd(211, ring, 2, 4099, ctx.RE), _rnd(212, ring, 2, 4099, ctx.RE)
    assert (ctx.ring_mul(a, b, form="coeff") == _through_ntt(ctx, a, b)).all()


# ---- 3. reduction corners -----------------------------------------------------------------------------------------------------------------------------------------------
def _corner_rows(kind, ring, nt, count, RE):
    p = RINGS[ring][0]
    if kind == "corner":
        return fc.table("corner", 301, (nt, count, RE), ring), fc.corner_table(302, (nt, count, RE), ring)
    if kind == "edge":                                 # every pair of grid words meets in some slot coordinate: rows of one word against rows that cycle the grid
        g = np.array(fc.EDGE_G if ring == "goldilocks" else fc.EDGE_B, dtype=np.uint64)
        a = np.repeat(g[np.arange(nt * count) % len(g)], RE).reshape(nt, count, RE)
        b = g[(np.arange(nt * count * RE) // 3) % len(g)].reshape(nt, count, RE)
        return a, b
    v = {"pm1": p - 1, "halfm": (p - 1) // 2, "halfp": (p + 1) // 2}[kind]
    full = np.full((nt, count, RE), v, dtype=np.uint64)
    return full, full.copy()


@pytest.mark.parametrize("kind", ["pm1", "halfm", "halfp", "corner", "edge"])
def test_reduction_corners_in_both_forms(rc, kind):
    """33 terms of the largest operands: the worst case of every sum whose reduction waits for the end of the terms"""
    ring, ctx = rc
    a, b = _corner_rows(kind, ring, 33, 5, ctx.RE)
    assert (ctx.ring_mul(a, b) == ntt_sum_bigint(a, b, ring)).all(), (ring, kind, "ntt")
    assert (ctx.ring_mul(a, b, form="coeff") == coeff_sum_bigint(a, b, ring)).all(), (ring, kind, "coeff")
    ad, bd = dev(a), dev(b)
    assert (host(ctx.ring_mul(ad, bd)) == ctx.ring_mul(a, b)).all() and (host(ctx.ring_mul(ad, bd, form="coeff")) == ctx.ring_mul(a, b, form="coeff")).all()


# ---- 4. units and zero divisors -----------------------------------------------------------------------------------------------------------------------------------------
def test_units_and_zero_divisors(rc):
    ring, ctx = rc
    p, d, tau = RINGS[ring]
    a = _rnd(401, ring, 67, d)
    one_ntt, zero = np.tile(diag(1, ring), (67, 1)), np.zeros((67, d), dtype=np.uint64)
    one_coeff = zero.copy()
    one_coeff[:, 0] = 1
    assert (ctx.ring_mul(a, one_ntt) == a).all() and (ctx.ring_mul(one_ntt, a) == a).all()
    assert (ctx.ring_mul(a, one_coeff, form="coeff") == a).all() and (ctx.ring_mul(one_coeff, a, form="coeff") == a).all()
    assert not ctx.ring_mul(a, zero).any() and not ctx.ring_mul(zero, a, form="coeff").any()
    x_top, x_1, want = (np.zeros((1, d), dtype=np.uint64) for _ in range(3))
    x_top[0, d - 1], x_1[0, 1] = 1, 1
    want[0, d // 2], want[0, 0] = 1, p - 1                      # X^(d-1) * X = X^d = X^(d/2) - 1
    assert (ctx.ring_mul(x_top, x_1, form="coeff") == want).all()
    u, v = a.copy(), _rnd(402, ring, 67, d)
    u[:, 2 * tau:3 * tau] = 0                                  # slot 2 of u is zero, every other slot of v is: u v = 0 although neither is
    v[:, :2 * tau] = 0
    v[:, 3 * tau:] = 0
    assert u.any() and v.any() and not ctx.ring_mul(u, v).any()


# ---- 5. the _dev twin ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["ntt", "coeff"])
def test_dev_twin_equals_the_host_call(rc, form):
    ring, ctx = rc
    for count, nt in ((67, 1), (259, 3)):
        a, b = _rnd(501 + count, ring, nt, count, ctx.RE), _rnd(502 + count, ring, nt, count, ctx.RE)
        want = ctx.ring_mul(a, b, form=form)
        ad, bd = dev(a), dev(b)
        got = ctx.ring_mul(ad, bd, form=form)
        assert (host(got) == want).all(), (ring, form, count, nt)
        assert (host(ad) == a).all() and (host(bd) == b).all(), "an input was written"
        o = blank(count, ctx.RE)
        assert ctx.ring_mul(ad, bd, form=form, out=o) is o and (host(o) == want).all()
    # in place: out = a, then out = b, one term; and a square (a and b the same array)
    a, b = _rnd(511, ring, 259, ctx.RE), _rnd(512, ring, 259, ctx.RE)
    want = ctx.ring_mul(a, b, form=form)
    ad, bd = dev(a), dev(b)
    assert ctx.ring_mul(ad, bd, form=form, out=ad) is ad and (host(ad) == want).all() and (host(bd) == b).all()
    ad = dev(a)
    assert ctx.ring_mul(ad, bd, form=form, out=bd) is bd and (host(bd) == want).all() and (host(ad) == a).all()
    assert (host(ctx.ring_mul(ad, ad, form=form)) == ctx.ring_mul(a, a, form=form)).all()


def test_dev_twin_refuses_overlaps_bad_pointers_and_bad_words(rc):
    ring, ctx = rc
    L, RE, p = api._lib(), ctx.RE, RINGS[ring][0]
    count, nbytes = 67, 67 * ctx.RE * 8
    a, b = _rnd(521, ring, 2, count, RE), _rnd(522, ring, 2, count, RE)
    ad, bd, o = dev(a), dev(b), blank(count, RE)
    call = lambda pa, pb, nt, po, form=0: L.lf_ring_mul_device(ctx.h, pa, pb, nt, count, form, po)
    hip, raw = _hip(), []
    try:
        for form in (0, 1):
            # two terms: out on table 0 of a, on table 1 of b, one element into a
            assert call(ad.data_ptr(), bd.data_ptr(), 2, ad.data_ptr(), form) == INVALID
            assert call(ad.data_ptr(), bd.data_ptr(), 2, bd.data_ptr() + nbytes, form) == INVALID
            assert call(ad.data_ptr(), bd.data_ptr(), 2, ad.data_ptr() + RE * 8, form) == INVALID
            # one term: a partial overlap is refused, out == a is not (tested above)
            assert call(ad.data_ptr(), bd.data_ptr(), 1, ad.data_ptr() + RE * 8, form) == INVALID
            host_arr = np.zeros(2 * count * RE, dtype=np.uint64)
            pinned = torch.zeros(2 * count * RE, dtype=torch.int64).pin_memory()
            for arg, size in (("a", 2 * nbytes), ("b", 2 * nbytes), ("out", nbytes)):
                short = C.c_void_p()
                assert hip.hipMalloc(C.byref(short), size - RE * 8) == 0      # one element short of the range the call touches
                raw.append(short)
                good = {"a": ad.data_ptr(), "b": bd.data_ptr(), "out": o.data_ptr()}
                for why, q in (("numpy", host_arr.ctypes.data), ("pinned", pinned.data_ptr()), ("misaligned", good[arg] + 4), ("short", short.value)):
                    ptrs = dict(good, **{arg: q})
                    assert call(ptrs["a"], ptrs["b"], 2, ptrs["out"], form) == INVALID, (ring, form, arg, why)
            assert not host_arr.any() and not pinned.numpy().any()
            # one word = p, in the first table of a and in the last word of b
            for which, pos in ((0, 0), (1, 2 * count * RE - 1)):
                bufs = [dev(a), dev(b)]
                bufs[which].view(-1)[pos] = np.array(p, dtype=np.uint64).view(np.int64).item()
                assert call(bufs[0].data_ptr(), bufs[1].data_ptr(), 2, o.data_ptr(), form) == INVALID, (ring, form, which)
                assert untouched(o)
        assert (host(ad) == a).all() and (host(bd) == b).all() and untouched(o)
    finally:
        for q in raw:
            hip.hipFree(q)
    # the context goes on working: case 1 at 67 elements, from device memory too
    want = ntt_sum_numpy(a, b, ring)
    assert (ctx.ring_mul(a, b) == want).all() and (host(ctx.ring_mul(ad, bd, out=o)) == want).all()


# ---- 6. external basis --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,kind", [("goldilocks", "random"), ("babybear", "random"), ("babybear", "tower")])      # (the tower basis is one of F_{p^9})
def test_external_basis(ring, kind):
    p = RINGS[ring][0]
    T = tower_T() if kind == "tower" else random_T(ring, 4242)
    Ti = _inv_matrix(T, p)
    ctx = api.Context(0, ring=ring)
    try:
        a, b = _rnd(601, ring, 3, 259, ctx.RE), _rnd(602, ring, 3, 259, ctx.RE)
        coeff_want = ctx.ring_mul(a, b, form="coeff")
        ctx.set_ext_basis(T)
        want = slotwise(T, ntt_sum_numpy(slotwise(Ti, a, ring), slotwise(Ti, b, ring), ring), ring)
        assert (ctx.ring_mul(a, b) == want).all(), (ring, kind)
        assert (host(ctx.ring_mul(dev(a), dev(b))) == want).all(), (ring, kind, "dev")
        assert (ctx.ring_mul(a, b, form="coeff") == coeff_want).all(), "coefficients have no basis"
        assert (host(ctx.ring_mul(dev(a), dev(b), form="coeff")) == coeff_want).all()
    finally:
        ctx.close()


# ---- 7. argument errors, bare and loaded contexts ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(rc):
    ring, ctx = rc
    L, RE = api._lib(), ctx.RE
    a = _rnd(701, ring, 4, RE)
    o = np.full((4, RE), SENTINEL, dtype=np.uint64)
    pa, po = a.ctypes.data_as(api.u64p), o.ctypes.data_as(api.u64p)
    ad, od = dev(a), blank(4, RE)
    assert L.lf_ring_mul(ctx.h, pa, pa, 0, 4, 0, po) == INVALID and L.lf_ring_mul_device(ctx.h, ad.data_ptr(), ad.data_ptr(), 0, 4, 0, od.data_ptr()) == INVALID
    assert L.lf_ring_mul(ctx.h, pa, pa, 1, 4, 2, po) == INVALID and L.lf_ring_mul_device(ctx.h, ad.data_ptr(), ad.data_ptr(), 1, 4, 2, od.data_ptr()) == INVALID
    assert L.lf_ring_mul(ctx.h, pa, pa, 1, 4, -1, po) == INVALID
    assert L.lf_ring_mul(ctx.h, pa, pa, 1, 4, 0, None) == INVALID and L.lf_ring_mul_device(ctx.h, ad.data_ptr(), ad.data_ptr(), 1, 4, 0, None) == INVALID
    assert L.lf_ring_mul(ctx.h, None, pa, 1, 4, 0, po) == INVALID and L.lf_ring_mul(ctx.h, pa, None, 1, 4, 0, po) == INVALID
    assert L.lf_ring_mul(None, pa, pa, 1, 4, 0, po) == INVALID
    assert (o == SENTINEL).all() and untouched(od)
    with pytest.raises(KeyError):
        ctx.ring_mul(a, a, form="mixed")
    assert L.lf_ring_mul(ctx.h, pa, pa, 1, 4, 0, po) == 0 and (o == ring_mul_ntt(a, a, ring)).all()       # the bare context accepts the call
    assert L.lf_ring_mul(ctx.h, pa, pa, 1, 0, 0, po) == L.lf_ntt_fwd(ctx.h, pa, po, 0)                     # count 0: what lf_ntt_fwd makes of it


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_products_around_a_fold_step(ring):
    """a context with a constraint system and a matrix computes the same words before and after a fold step, and the step's proof is still the oracle's: the
    product shares no scratch with the step"""
    O = _oracle(ring)
    wl = make_workload(NAMES[ring])
    inst = O.Instance(wl)
    ctx = api.Context(0, ring=ring)
    try:
        a, b = _rnd(711, ring, 3, 259, ctx.RE), _rnd(712, ring, 3, 259, ctx.RE)
        want = {f: ctx.ring_mul(a, b, form=f) for f in FORM}
        assert (want["ntt"] == ntt_sum_numpy(a, b, ring)).all()
        ctx.load_ccs(wl)
        Aw = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=Aw)
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        f_coeff = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        tr = lambda: api.PoseidonTranscript(ring=ring)
        for f in FORM:
            assert (ctx.ring_mul(a, b, form=f) == want[f]).all(), (ring, f, "loaded")
        acc, _lin = api.LFLinearizationProver.prove(ctx, cccs, wit, tr())
        acc_o, _lin_o = inst.linearize(O.Transcript(), cccs, f_coeff)
        assert (host(ctx.ring_mul(dev(a), dev(b))) == want["ntt"]).all()
        lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr())
        lc_o, f0_o, proof_o = inst.fold_step(O.Transcript(), Aw, acc_o, f_coeff, cccs, f_coeff)
        assert (proof == proof_o).all() and (lc == lc_o).all() and (w0.f == f0_o).all()
        for f in FORM:
            assert (ctx.ring_mul(a, b, form=f) == want[f]).all(), (ring, f, "after the step")
            assert (host(ctx.ring_mul(dev(a), dev(b), form=f)) == want[f]).all()
    finally:
        ctx.close()


# ---- 8. a use: the gate values of a degree-five constraint system, on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T10", "B8"])
def test_z_to_the_fourth_on_the_device(name):
    wl = make_workload(name, ccs="deg5")
    rows = min(wl.n, wl.m)
    ctx = api.Context(0, ring=wl.ring)
    try:
        z = dev(wl.z()[:rows])
        z2 = ctx.ring_mul(z, z)
        z4 = ctx.ring_mul(z2, z2, out=z2)
        assert (host(z4) == wl.val[5][:rows]).all()
    finally:
        ctx.close()
