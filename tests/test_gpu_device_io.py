"""Device-resident callers: the `_dev` entry points of include/lfhip.h take and return the O(n) arrays as memory of the context's device (torch tensors here),
read and written in place by the relayout kernels.  Every comparison is exact equality of words: with the host-pointer twin of the call and with the CPU oracle.

Shapes: counts 1, 63, 64, 65, 200 around the 64-element tile of the relayout block (one element, a ragged single block, a full block, one element into the
second block, a ragged fourth block); T8 / B6 (N = 256 / 64) and R61b4 (N = 244, ragged) for the commitments; T8, B6, T8b4 for whole steps; T12/general5 for the
general CSR rows, which gather from the caller's buffer itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from latticefold_amd import api
from latticefold_amd.workload import CONFIGS, RINGS, make_workload, splitmix_fq
from test_gpu_wide_ccs import _sections, general_deg5
from test_relation_check_cpu import bad_rows, residual_host

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
COUNTS = (1, 63, 64, 65, 200)


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


def _rnd(seed, ring, *shape):
    return splitmix_fq(seed, 0, int(np.prod(shape)), ring).reshape(shape).copy()


def _tr(ring):
    return api.PoseidonTranscript(ring=ring)


def _relayout_case(ctx, ring, count):
    """case 1 for one count: crt / icrt from and into device arrays, out of place and in place, against the host-pointer call and the oracle"""
    O = _oracle(ring)
    x = _rnd(1000 + count, ring, count, ctx.RE)
    for fn, ofn in ((ctx.ntt_fwd, O.crt), (ctx.ntt_inv, O.icrt)):
        want = ofn(x)
        assert (fn(x) == want).all(), (ring, count, "host-pointer call")
        src = dev(x)
        got = fn(src)
        assert (host(got) == want).all(), (ring, count, "device call")
        assert (host(src) == x).all(), (ring, count, "the input was written")
        assert fn(src, out=src) is src and (host(src) == want).all(), (ring, count, "in place")


@pytest.fixture(scope="module", params=["goldilocks", "babybear"])
def ring_ctx(request):
    ctx = api.Context(0, ring=request.param)
    yield request.param, ctx
    ctx.close()


# ---- 1. relayout edges ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_ntt_on_device_arrays(ring_ctx, count):
    ring, ctx = ring_ctx
    _relayout_case(ctx, ring, count)


def test_ntt_partial_overlap_is_refused(ring_ctx):
    ring, ctx = ring_ctx
    L = api._lib()
    buf = dev(_rnd(3, ring, 66, ctx.RE))
    before = host(buf).copy()
    p = buf.data_ptr()
    for fn in (L.lf_ntt_fwd_dev, L.lf_ntt_inv_dev):
        assert fn(ctx.h, p, p + ctx.RE * 8, 65) == INVALID       # out one element behind in
        assert fn(ctx.h, p + ctx.RE * 8, p, 65) == INVALID
        assert fn(ctx.h, p, p + 65 * ctx.RE * 8, 1) == 0          # disjoint halves of one allocation are fine
    after = host(buf)
    assert (after[:65] == before[:65]).all()


# ---- 2. commitments ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T8", "R61b4", "B6"])
def test_commits_from_device_arrays(name):
    wl = make_workload(name)
    ring = wl.ring
    O = _oracle(ring)
    ctx = api.Context(0, ring=ring)
    try:
        A = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        N, L, B, kappa = wl.N, wl.L, wl.B, wl.kappa
        for batch in (1, 2):
            f = _rnd(10 + batch, ring, batch, N, ctx.RE)
            want = np.stack([O.ajtai_commit(A, kappa, N, x) for x in f])
            assert (scheme.commit(f) == want).all() and (scheme.commit(dev(f)) == want).all(), (name, batch, "commit")
            want = np.stack([O.ajtai_commit(A, kappa, N, O.crt(x)) for x in f])
            assert (scheme.commit_coeff(f) == want).all() and (scheme.commit_coeff(dev(f)) == want).all(), (name, batch, "commit_coeff")
            g = _rnd(20 + batch, ring, batch, N // L, ctx.RE)
            want = np.stack([O.ajtai_commit(A, kappa, N, O.crt(O.decompose(x, B, L, 0))) for x in g])
            assert (scheme.decompose_and_commit_coeff(g, B, L) == want).all(), (name, batch, "host decompose_and_commit_coeff")
            assert (scheme.decompose_and_commit_coeff(dev(g), B, L) == want).all(), (name, batch, "decompose_and_commit_coeff")
            gn = np.stack([O.crt(x) for x in g])
            assert (scheme.decompose_and_commit_ntt(gn, B, L) == want).all(), (name, batch, "host decompose_and_commit_ntt")
            assert (scheme.decompose_and_commit_ntt(dev(gn), B, L) == want).all(), (name, batch, "decompose_and_commit_ntt")
        # a single vector (n, d) as well as a batch of one
        assert (scheme.commit(dev(f[0])) == O.ajtai_commit(A, kappa, N, f[0])).all()
        with pytest.raises(api.CommitmentError):
            scheme.commit(dev(f[0][:-1]))
    finally:
        ctx.close()


# ---- 3. witnesses and a whole step -----------------------------------------------------------------------------------------------------------------------------
def _getters(w):
    return w.f_coeff, w.f, w.w_ccs


@pytest.mark.parametrize("name", ["T8", "B6", "T8b4"])
def test_witnesses_and_a_fold_step_from_device_memory(name):
    wl = make_workload(name)
    ring = wl.ring
    O = _oracle(ring)
    ctx = api.Context(0, ring=ring)
    try:
        ctx.load_ccs(wl)
        A = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        inst = O.Instance(wl)
        f = inst.witness_from_w_ccs(wl.w_ccs)                       # coefficient form, (N, d)
        w_host = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        want = _getters(w_host)
        assert (want[0] == f).all() and (want[1] == O.crt(f)).all() and (want[2] == wl.w_ccs).all()
        w_a = api.Witness.from_w_ccs(ctx, dev(wl.w_ccs))
        w_b = api.Witness.from_f_coeff(ctx, dev(f))
        w_c = api.Witness.from_f(ctx, dev(O.crt(f)))
        for w, how in ((w_a, "from_w_ccs"), (w_b, "from_f_coeff"), (w_c, "from_f")):
            assert all((g == h).all() for g, h in zip(_getters(w), want)), (name, how)
        assert all((g == h).all() for g, h in zip(_getters(api.Witness.from_f_coeff(ctx, f)), want))
        assert all((g == h).all() for g, h in zip(_getters(api.Witness.from_f(ctx, O.crt(f))), want))

        # NIFSProver::prove with both witnesses ingested from device memory, against the oracle's
        cccs = np.concatenate([w_a.commit(scheme), wl.x_ccs])
        acc, lin = api.LFLinearizationProver.prove(ctx, cccs, w_a, _tr(ring))
        lc, w0, proof = api.NIFSProver.prove(ctx, acc, w_a, cccs, w_b, _tr(ring))
        cccs_o = np.concatenate([O.ajtai_commit(A, wl.kappa, wl.N, O.crt(f)), wl.x_ccs])
        acc_o, lin_o = inst.linearize(O.Transcript(), cccs_o, f)
        lc_o, f0_o, proof_o = inst.fold_step(O.Transcript(), A, acc_o, f, cccs_o, f)
        assert (cccs == cccs_o).all() and (lin == lin_o).all() and (acc == acc_o).all()
        so, sg = _sections(wl, proof_o), _sections(wl, proof)
        bad = [k for k in so if so[k].shape != sg[k].shape or not (so[k] == sg[k]).all()]
        assert not bad, f"{name}: proof sections differing from the oracle: {bad}"
        assert (lc == lc_o).all() and (w0.f == f0_o).all() and (w0.f_coeff == O.icrt(f0_o)).all()

        # the folded witness through the three device getters
        mk = lambda rows: torch.full((rows, ctx.RE), -1, dtype=torch.int64, device="cuda")
        assert (host(w0.f_into(mk(wl.N))) == w0.f).all()
        assert (host(w0.f_coeff_into(mk(wl.N))) == w0.f_coeff).all()
        assert (host(w0.w_ccs_into(mk(wl.wit_len))) == w0.w_ccs).all()
        assert (host(w_a.f_into(mk(wl.N))) == want[1]).all()          # (a handle without a cached NTT form)
        assert (host(w_a.w_ccs_into(mk(wl.wit_len))) == wl.w_ccs).all()
    finally:
        ctx.close()


# ---- 4. check_relation from a device z -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ccs", [("T8", "r1cs"), ("T12", "general5"), ("B6", "r1cs")])
def test_check_relation_from_a_device_z(name, ccs):
    wl = general_deg5(name) if ccs == "general5" else make_workload(name, ccs=ccs)
    if ccs == "general5":   # the general CSR layout: k_spmv_rows gathers whole elements from the caller's buffer
        assert int(wl.rowptr[0][-1]) * 2 > min(wl.n, wl.m) * 3
    p = RINGS[wl.ring][0]
    ctx = api.Context(0, ring=wl.ring)
    try:
        ctx.load_ccs(wl)
        z = wl.z()
        zd = dev(z)
        assert ctx.check_relation(z) is None and ctx.check_relation(zd) is None
        assert (host(zd) == z).all()
        bad = z.copy()
        col = wl.l + 1 + 7
        bad[col, 0] = (int(bad[col, 0]) + 1) % p
        rows = bad_rows(residual_host(wl, bad))
        assert rows.size
        for arg in (bad, dev(bad)):
            with pytest.raises(api.NotSatisfied) as e:
                ctx.check_relation(arg)
            assert e.value.row == int(rows[0])
    finally:
        ctx.close()


# ---- 5. ordering -----------------------------------------------------------------------------------------------------------------------------------------------
def test_input_produced_on_another_torch_stream(ring_ctx):
    """the input is still being written by kernels of a non-default torch stream when the call is made: api orders the context behind that stream
    (lf_ctx_wait_stream), nobody synchronises"""
    ring, ctx = ring_ctx
    count = 1 << 13
    x = _rnd(77, ring, count, ctx.RE)
    want = ctx.ntt_fwd(x)
    base = dev(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = base.clone()
        for _ in range(8):
            t += 12345
            t -= 12345
        got = ctx.ntt_fwd(t)
        again = ctx.ntt_fwd(t, out=t)
    assert (host(got) == want).all() and (host(again) == want).all()


# ---- 6. refusals: nothing of these may reach a kernel ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def n65(monkeypatch):
    """a constraint system whose witness vectors have 65 elements (one element into the second relayout block)"""
    monkeypatch.setitem(CONFIGS, "N65", (7, 65, 1, 1 << 16, 2, 16, 2))
    return make_workload("N65")


def test_refusals(n65):
    wl = n65
    ring, O, L = wl.ring, _oracle(wl.ring), api._lib()
    p = RINGS[ring][0]
    ctx = api.Context(0, ring=ring)
    try:
        ctx.load_ccs(wl)
        RE, n = ctx.RE, 65
        assert (wl.N, wl.wit_len) == (n, n)
        A = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        small = (_rnd(5, ring, n, RE) % np.uint64(7)).astype(np.uint64)          # coefficients inside the bound B / 2
        wit = api.Witness.from_f_coeff(ctx, small)
        good = dev(O.crt(small))
        out = torch.full((n, RE), -1, dtype=torch.int64, device="cuda")
        cm = np.zeros((wl.kappa, RE), dtype=np.uint64)
        pcm = cm.ctypes.data_as(api.u64p)
        h = C.c_void_p()
        fb = C.c_uint64()
        pfb = C.cast(C.byref(fb), api.u64p)
        pinned = torch.zeros((n, RE), dtype=torch.int64).pin_memory()
        zbad = {"null": None, "pinned host": pinned.data_ptr(), "misaligned": good.data_ptr() + 4}
        for why, q in zbad.items():
            g, o = good.data_ptr(), out.data_ptr()
            rcs = {"ntt_fwd in": L.lf_ntt_fwd_dev(ctx.h, q, o, n), "ntt_fwd out": L.lf_ntt_fwd_dev(ctx.h, g, q, n),
                   "ntt_inv in": L.lf_ntt_inv_dev(ctx.h, q, o, n), "ntt_inv out": L.lf_ntt_inv_dev(ctx.h, g, q, n),
                   "commit": L.lf_ajtai_commit_dev(ctx.h, q, n, 1, pcm), "commit_coeff": L.lf_ajtai_commit_coeff_dev(ctx.h, q, n, 1, pcm),
                   "dec_coeff": L.lf_ajtai_decompose_and_commit_coeff_dev(ctx.h, q, n, 1 << 16, 1, 1, pcm),
                   "dec_ntt": L.lf_ajtai_decompose_and_commit_ntt_dev(ctx.h, q, n, 1 << 16, 1, 1, pcm),
                   "from_w_ccs": L.lf_witness_from_w_ccs_dev(ctx.h, q, C.byref(h)), "from_f_coeff": L.lf_witness_from_f_coeff_dev(ctx.h, q, C.byref(h)),
                   "from_f": L.lf_witness_from_f_dev(ctx.h, q, C.byref(h)),
                   "get_f": L.lf_witness_get_f_dev(ctx.h, wit.h, q), "get_f_coeff": L.lf_witness_get_f_coeff_dev(ctx.h, wit.h, q),
                   "get_w_ccs": L.lf_witness_get_w_ccs_dev(ctx.h, wit.h, q)}
            assert all(rc == INVALID for rc in rcs.values()), (why, rcs)
            assert not h.value
        for why, q in zbad.items():     # z has n = l + 1 + wit_len = 67 elements: its own buffers
            zp = torch.zeros((wl.n, RE), dtype=torch.int64).pin_memory()
            zq = {"null": None, "pinned host": zp.data_ptr(), "misaligned": dev(wl.z()).data_ptr() + 4}[why]
            assert L.lf_ccs_check_dev(ctx.h, zq, pfb) == INVALID, why
        assert (host(out) == np.uint64(2**64 - 1)).all() and not cm.any() and not pinned.numpy().any()

        # a word >= p in the last word of the last element: refused by the device's own check, nothing written, no handle
        for word in (p, 2**64 - 1):
            x = O.crt(small)
            x[-1, -1] = word
            xd = dev(x)
            assert L.lf_ntt_fwd_dev(ctx.h, xd.data_ptr(), out.data_ptr(), n) == INVALID, word
            assert L.lf_ntt_fwd_dev(ctx.h, xd.data_ptr(), xd.data_ptr(), n) == INVALID and (host(xd) == x).all(), word
            assert L.lf_ajtai_commit_dev(ctx.h, xd.data_ptr(), n, 1, pcm) == INVALID, word
            assert L.lf_witness_from_f_dev(ctx.h, xd.data_ptr(), C.byref(h)) == INVALID and not h.value, word
            zz = wl.z()
            zz[-1, -1] = word
            assert L.lf_ccs_check_dev(ctx.h, dev(zz).data_ptr(), pfb) == INVALID, word
            assert (host(out) == np.uint64(2**64 - 1)).all() and not cm.any()
        # the first word of the first element as well (the other end of the grid)
        x = O.crt(small)
        x[0, 0] = p
        assert L.lf_ntt_inv_dev(ctx.h, dev(x).data_ptr(), out.data_ptr(), n) == INVALID
        assert (host(out) == np.uint64(2**64 - 1)).all()

        # the same context goes on working
        for count in COUNTS:
            _relayout_case(ctx, ring, count)
        assert (scheme.commit(good) == O.ajtai_commit(A, wl.kappa, n, O.crt(small))).all()
        w2 = api.Witness.from_f(ctx, good)
        assert (w2.f_coeff == small).all()
        assert ctx.check_relation(dev(wl.z())) is None
    finally:
        ctx.close()


def test_state_and_length_errors_are_the_host_twins():
    wl = make_workload("T8")
    ctx = api.Context(0)
    try:
        L = api._lib()
        t = dev(_rnd(1, "goldilocks", wl.N, 24))
        cm = np.zeros((wl.kappa, 24), dtype=np.uint64)
        h, fb = C.c_void_p(), C.c_uint64()
        assert L.lf_ajtai_commit_dev(ctx.h, t.data_ptr(), wl.N, 1, cm.ctypes.data_as(api.u64p)) == STATE          # no matrix
        assert L.lf_witness_from_f_dev(ctx.h, t.data_ptr(), C.byref(h)) == STATE                                   # no constraint system
        assert L.lf_ccs_check_dev(ctx.h, t.data_ptr(), C.cast(C.byref(fb), api.u64p)) == STATE
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=wl.ajtai_matrix())
        assert L.lf_ajtai_commit_dev(ctx.h, t.data_ptr(), wl.N - 1, 1, cm.ctypes.data_as(api.u64p)) == INVALID     # WrongWitnessLength
        assert L.lf_ajtai_decompose_and_commit_coeff_dev(ctx.h, t.data_ptr(), wl.N // 4, 3, 4, 1, cm.ctypes.data_as(api.u64p)) == -3   # base 3
        assert scheme.width() == wl.N
    finally:
        ctx.close()


# ---- 7. the host-pointer paths next to the device ones ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T8", "B6"])
def test_host_pointer_calls_interleaved_with_device_calls(name):
    wl = make_workload(name)
    ring = wl.ring
    O = _oracle(ring)
    ctx = api.Context(0, ring=ring)
    try:
        ctx.load_ccs(wl)
        A = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        f = O.Instance(wl).witness_from_w_ccs(wl.w_ccs)
        x = _rnd(9, ring, 200, ctx.RE)
        v = _rnd(8, ring, wl.N, ctx.RE)
        want_cm = O.ajtai_commit(A, wl.kappa, wl.N, v)
        for rep in range(2):
            assert (ctx.crt(x) == O.crt(x)).all()
            assert (host(ctx.crt(dev(x))) == O.crt(x)).all()
            assert (ctx.icrt(x) == O.icrt(x)).all()
            assert (scheme.commit(v) == want_cm).all()
            assert (scheme.commit(dev(v)) == want_cm).all()
            assert (scheme.commit_coeff(v) == O.ajtai_commit(A, wl.kappa, wl.N, O.crt(v))).all()
            wd = api.Witness.from_w_ccs(ctx, dev(wl.w_ccs))
            wh = api.Witness.from_w_ccs(ctx, wl.w_ccs)
            assert (wh.f_coeff == f).all() and (wh.f == O.crt(f)).all() and (wh.w_ccs == wl.w_ccs).all()
            assert (host(wd.f_into(torch.empty((wl.N, ctx.RE), dtype=torch.int64, device="cuda"))) == wh.f).all()
            assert (wh.commit(scheme) == O.ajtai_commit(A, wl.kappa, wl.N, O.crt(f))).all()
            assert ctx.check_relation(wl.z()) is None and ctx.check_relation(dev(wl.z())) is None
    finally:
        ctx.close()
