"""Device-resident callers of the LatticeFold+ ABI: the `_dev` twins of include/lfplus.h take and return the O(n) arrays -- the witness f, the short witness z,
the vector of lfplus_commit, the halves F0 / F1 -- as memory of the context's device (torch tensors here), in the layout of the host ABI, and
lfplus_ctx_wait_stream / lfplus_prover_wait_stream order a context or a prover behind the stream that produced them.  Every result is compared word for word
with the host-pointer twin and with the oracle (oracle/lfp.c through tests/lfp.py); the prover chain with the host-pointer chain, which
tests/test_gpu_lfplus_native.py pins to the oracle.  Bit-exact: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import lfp
from latticefold_amd import plus
from test_gpu_lfplus_ingest import _patterns, _rg_read
from test_gpu_lfplus_native import N, _shape, _zs

pytestmark = pytest.mark.gpu
D, P = 16, plus.P
E_ARG = plus.E_ARG
SENT = 0x5A5A5A5A5A5A5A5A
u64p = plus.u64p


def L():
    return plus._nlib()


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda")
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint64)


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def dsent(*shape):
    """a device array filled with the sentinel, complete before the library's streams may look at it"""
    t = torch.full(shape, SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def hsent(*shape):
    return np.full(shape, SENT, dtype=np.uint64)


def hp(a):
    return a.ctypes.data_as(u64p)


def untouched(*arrays):
    return all(((host(a) if torch.is_tensor(a) else a) == SENT).all() for a in arrays)


# ---- 1. components ---------------------------------------------------------------------------------------------------------------------------------------------
# (kappa, k, b, n) of tests/test_gpu_lfplus_ingest.py: two shapes under one tile of 16 z elements, two that end inside a tile, 2^12 and 2^15 rows
COMPONENT_CASES = [(1, 16, 2, 64), (5, 4, 3108, 64), (2, 3, 7, 111), (1, 4, 16, 400), (2, 4, 3108, 4096), (1, 4, 8, 1 << 15)]


@pytest.mark.parametrize("kappa,k,b,n", COMPONENT_CASES)
def test_components_match_the_host_twins_and_the_oracle(kappa, k, b, n):
    """witness_from_z_dev / get_witness_dev / commit_dev / set_witness_dev + commit_resident; n = 111 passes element-granular views at a non-zero offset inside
    larger tensors"""
    m, views = n // k, n == 111
    A = lfp.splitmix(40 + kappa, 0, kappa * n * D).reshape(kappa, n, D)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        for name, z in _patterns(b, k, m, n + k).items():
            cm_h = ctx.witness_from_z(z, b, k)
            f_h = ctx.get_witness()
            slow = name == "random" and n >= 1 << 12          # (the oracle binding builds a table per distinct value)
            want = plus.gadget_decompose(z, b, k) if slow else lfp.gadget_decompose(z, b, k)
            cm_o = lfp.commit(A, want)
            assert (f_h == want).all() and (cm_h == cm_o).all(), (name, "host twin against the oracle")
            if views:
                zbig, fbig = dsent(m + 5, D), dsent(n + 3, D)
                zbig[3:3 + m] = dev(z)
                zd, fd = zbig[3:3 + m], fbig[1:1 + n]
                assert zd.data_ptr() == zbig.data_ptr() + 3 * 128 and fd.data_ptr() == fbig.data_ptr() + 128 and zd.is_contiguous() and fd.is_contiguous()
            else:
                zd, fd = dev(z), dsent(n, D)
            torch.cuda.synchronize()
            ctx.set_witness(np.zeros((n, D), dtype=np.uint64))      # (another witness: what follows must replace it)
            cm = hsent(kappa, D)
            assert L().lfplus_witness_from_z_dev(ctx.h, ptr(zd), m, b, k, hp(cm)) == 0, plus._lib().lfplus_last_error(ctx.h)
            assert (cm == cm_o).all(), (name, "cm_f")
            assert L().lfplus_get_witness_dev(ctx.h, ptr(fd), n) == 0
            assert (host(fd) == want).all(), (name, "f")
            out = hsent(kappa, D)
            assert L().lfplus_commit_dev(ctx.h, ptr(fd), n, hp(out)) == 0
            assert (out == cm_o).all(), (name, "commit_dev")
            ctx.set_witness(np.zeros((n, D), dtype=np.uint64))
            assert L().lfplus_set_witness_dev(ctx.h, ptr(fd), n) == 0
            assert (ctx.commit_resident() == cm_o).all(), (name, "set_witness_dev + commit_resident")
            assert (ctx.get_witness() == want).all(), (name, "set_witness_dev")
            assert (host(zd) == z).all() and (host(fd) == want).all(), (name, "the inputs are unchanged")
            if views:
                assert untouched(zbig[:3], zbig[3 + m:], fbig[:1], fbig[1 + n:]), (name, "outside the views")
            # the Python layer dispatches on the array's home
            assert (ctx.witness_from_z(zd, b, k) == cm_o).all() and (ctx.commit(fd) == cm_o).all()
            ctx.set_witness(fd)
            got = ctx.get_witness(out=dsent(n, D))
            assert (host(got) == want).all(), (name, "plus.py")
    finally:
        ctx.close()


# ---- 2. decompose ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kappa,resident", [(64, 1, False), (1 << 12, 2, True)])
def test_decompose_into_device_arrays(n, kappa, resident):
    """Decomp::decompose with F0 / F1 written into the caller's device arrays: against lfp.decompose and the host twin; then F0 NULL and F1 given"""
    B, nv = 50, n.bit_length() - 1
    A = lfp.splitmix(41, 0, kappa * n * D).reshape(kappa, n, D)
    v = (lfp.splitmix(42, 0, n * D) % np.uint64(2001)).astype(np.int64) - 1000
    f = np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)
    r = lfp.splitmix(43, 0, nv * 2 * D).reshape(nv, 2, D)
    mats = [plus.identity_csr(n)] * 3 if resident else []
    want = lfp.decompose(f, A, B, np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1]), mats)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        if resident:
            ctx.set_matrices(mats)
        M = plus.RESIDENT(3) if resident else ()
        ctx.set_witness(f)
        twin = ctx.decompose(None, None, B, r, M)
        F0, F1 = dsent(n, D), dsent(n, D)
        got = ctx.decompose(None, None, B, r, M, out=(F0, F1))
        assert got["F0"] is F0 and got["F1"] is F1
        for key in ("F0", "F1", "C0", "C1", "v0", "v1"):
            g = host(got[key]) if key in ("F0", "F1") else got[key]
            assert (g == want[key]).all() and (g == twin[key]).all(), key
        F1b = dsent(n, D)
        got = ctx.decompose(None, None, B, r, M, out=(None, F1b))
        assert got["F0"] is None and (host(F1b) == want["F1"]).all()
        for key in ("C0", "C1", "v0", "v1"):
            assert (got[key] == want[key]).all(), (key, "F0 NULL")
        assert (ctx.get_witness() == f).all(), "the decomposed witness stays resident"
    finally:
        ctx.close()


# ---- 3. refusals: nothing of these may reach a kernel ----------------------------------------------------------------------------------------------------------
def _bad_pointers(n):
    """[(name, address)]: NULL, pinned host memory, a device pointer + 4 and + 8 (8-byte but not 16-byte aligned), and a range that runs off its allocation -- 128
    bytes before the end of a tensor that is an allocation of its own (32 MiB, requested from an empty cache: nothing larger is there to be split)"""
    torch.cuda.empty_cache()
    big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")
    pinned = torch.zeros((n, D), dtype=torch.int64).pin_memory()
    good = torch.zeros((n + 1, D), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    keep = (big, pinned, good)
    return keep, [("null", None), ("pinned", pinned.data_ptr()), ("dev+4", good.data_ptr() + 4), ("dev+8", good.data_ptr() + 8),
                  ("off the end", big.data_ptr() + (32 << 20) - 128)]


def test_bad_pointers_are_refused_before_anything_is_touched():
    kappa, k, n = 1, 4, N
    A, r1cs, params = _shape(kappa, k)
    B, m, nv = params.B, n // k, n.bit_length() - 1
    z = _zs(k, (1,))[0][0]
    f = plus.gadget_decompose(z, B, k)
    r = lfp.splitmix(43, 0, nv * 2 * D).reshape(nv, 2, D)
    r_a, r_b = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    keep, bad = _bad_pointers(n)
    ctx = plus.PlusContext(0)
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        ctx.set_matrix(A)
        ctx.set_witness(f)
        cm0 = ctx.commit_resident()
        lib = L()

        def refused(rc, *sentinels):
            assert rc == E_ARG and plus._lib().lfplus_last_error(ctx.h), rc
            assert untouched(*sentinels)
            assert (ctx.commit_resident() == cm0).all(), "the resident witness is as it was"

        for name, addr in bad:
            p = C.c_void_p(addr)
            out, Fg = hsent(kappa, D), dsent(n, D)
            refused(lib.lfplus_set_witness_dev(ctx.h, p, n))
            refused(lib.lfplus_witness_from_z_dev(ctx.h, p, m, B, k, hp(out)), out)
            refused(lib.lfplus_commit_dev(ctx.h, p, n, hp(out)), out)
            refused(lib.lfplus_get_witness_dev(ctx.h, p, n))
            if addr is not None:         # (a NULL half is "not wanted", as in the host call)
                small = [hsent(kappa, D), hsent(kappa, D), hsent(1, 2, D), hsent(1, 2, D)]
                for F0, F1 in ((p, ptr(Fg)), (ptr(Fg), p)):
                    refused(lib.lfplus_decompose_dev(ctx.h, B, hp(r_a), hp(r_b), 0, None, None, None, F0, F1, *[hp(x) for x in small]), Fg, *small)
            # the prover: refused as a shape error -- not FAILED, nothing named for the next prove
            cms = hsent(1, kappa, D)
            arr = (C.c_void_p * 1)(addr)
            assert lib.lfplus_prover_ingest_dev(prover.h, arr, 1, m, 1, hp(cms)) == E_ARG and prover.last_error(), name
            assert lib.lfplus_prover_set_instances_dev(prover.h, arr, None, 1) == E_ARG and prover.last_error(), name
            assert untouched(cms)
        # F0 / F1 overlapping each other
        two = dsent(2 * n, D)
        small = [hsent(kappa, D), hsent(kappa, D), hsent(1, 2, D), hsent(1, 2, D)]
        refused(lib.lfplus_decompose_dev(ctx.h, B, hp(r_a), hp(r_b), 0, None, None, None, ptr(two), ptr(two, 128), *[hp(x) for x in small]), two, *small)
        refused(lib.lfplus_decompose_dev(ctx.h, B, hp(r_a), hp(r_b), 0, None, None, None, ptr(two, 128 * (n - 1)), ptr(two), *[hp(x) for x in small]), two, *small)
        # the prover is usable: one prove, then the accumulator's refusals, then the accumulator itself
        prover.ingest([z], r1cs)
        flat = prover.prove()
        assert plus.NativePlusVerifier.init(A, list(r1cs), params, plus.PoseidonTranscript()).verify(flat, 1, 1)
        Fg = dsent(n, D)
        for name, addr in bad[1:]:
            p = C.c_void_p(addr)
            assert lib.lfplus_prover_accumulator_dev(prover.h, p, ptr(Fg)) == E_ARG and prover.last_error(), name
            assert lib.lfplus_prover_accumulator_dev(prover.h, ptr(Fg), p) == E_ARG, name
            assert untouched(Fg)
        assert lib.lfplus_prover_accumulator_dev(prover.h, ptr(two), ptr(two, 128)) == E_ARG and untouched(two), "overlap"
        F0, F1 = prover.accumulator()
        got = prover.accumulator(out=(dsent(n, D), dsent(n, D)))
        assert (host(got[0]) == F0).all() and (host(got[1]) == F1).all()
    finally:
        prover.close()
        ctx.close()
        del keep
        plus.scratch_trim(0)


def test_a_sharded_context_refuses_every_device_call():
    kappa, k, n, B = 1, 4, 1 << 10, 16
    A = lfp.splitmix(44, 0, kappa * (n // 2) * D).reshape(kappa, n // 2, D)
    f = (lfp.splitmix(45, 0, n * D) % np.uint64(8)).reshape(n, D)
    nv = n.bit_length() - 1
    r = lfp.splitmix(43, 0, nv * 2 * D).reshape(nv, 2, D)
    r_a, r_b = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    ctx = plus.PlusContext(0)
    try:
        ctx.set_sharding_model(0, 2)
        ctx.set_matrix(A)
        ctx.set_witness(f)
        lib, fd, zd = L(), dev(f), dev(f[:n // k])
        out, Fo = hsent(kappa, D), dsent(n, D)
        small = [hsent(kappa, D), hsent(kappa, D), hsent(1, 2, D), hsent(1, 2, D)]
        assert lib.lfplus_set_witness_dev(ctx.h, ptr(fd), n) == E_ARG
        assert lib.lfplus_witness_from_z_dev(ctx.h, ptr(zd), n // k, B, k, hp(out)) == E_ARG
        assert lib.lfplus_commit_dev(ctx.h, ptr(fd), n, hp(out)) == E_ARG
        assert lib.lfplus_get_witness_dev(ctx.h, ptr(Fo), n) == E_ARG
        assert lib.lfplus_decompose_dev(ctx.h, B, hp(r_a), hp(r_b), 0, None, None, None, ptr(Fo), None, *[hp(x) for x in small]) == E_ARG
        assert untouched(out, Fo, *small)
        assert (ctx.get_witness() == f).all(), "the witness the host handed over is still there"
    finally:
        ctx.close()


# ---- 4. non-canonical words: the device finds them -------------------------------------------------------------------------------------------------------------
def _with_bad_word(a, where, value):
    a = np.array(a, dtype=np.uint64, copy=True)
    flat = a.reshape(-1)
    flat[{"first": 0, "middle": (flat.size // 2) | 1, "last": flat.size - 1}[where]] = np.uint64(value)
    return a


@pytest.mark.parametrize("value", [P, 2**64 - 1])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_non_canonical_words(value, where):
    kappa, k, b, n = 1, 4, 16, 400
    m = n // k
    A = lfp.splitmix(46, 0, kappa * n * D).reshape(kappa, n, D)
    z = lfp.splitmix(47, 0, m * D).reshape(m, D)
    f = plus.gadget_decompose(z, b, k)
    fbad, zbad = dev(_with_bad_word(f, where, value)), dev(_with_bad_word(z, where, value))
    ctx = plus.PlusContext(0)
    try:
        lib = L()
        ctx.set_matrix(A)
        ctx.set_witness(f)
        cm0, out, back = ctx.commit_resident(), hsent(kappa, D), hsent(n, D)
        assert lib.lfplus_commit_dev(ctx.h, ptr(fbad), n, hp(out)) == E_ARG and untouched(out)
        assert (ctx.commit_resident() == cm0).all() and (ctx.get_witness() == f).all(), "commit_dev leaves the witness alone"
        assert lib.lfplus_set_witness_dev(ctx.h, ptr(fbad), n) == E_ARG
        assert lib.lfplus_get_witness(ctx.h, hp(back), n) == E_ARG and untouched(back), "no resident witness after set_witness_dev failed"
        ctx.set_witness(f)
        assert lib.lfplus_witness_from_z_dev(ctx.h, ptr(zbad), m, b, k, None) == E_ARG
        assert lib.lfplus_get_witness(ctx.h, hp(back), n) == E_ARG and untouched(back), "no resident witness after witness_from_z_dev failed"
    finally:
        ctx.close()
    # the prover reports the word at once (no upload thread) and is FAILED afterwards
    A, r1cs, params = _shape(1, 4)
    fN = plus.gadget_decompose(_zs(4, (1,))[0][0], params.B, 4)
    bad = dev(_with_bad_word(fN, where, value))
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        arr = (C.c_void_p * 1)(bad.data_ptr())
        assert lib.lfplus_prover_set_instances_dev(prover.h, arr, None, 1) == E_ARG and "non-canonical" in prover.last_error()
        words = plus.proof_len(params, N, 3, 1, 1)
        proof = np.zeros(words, dtype=np.uint64)
        assert lib.lfplus_prover_prove(prover.h, hp(proof), words) == E_ARG and "failed earlier" in prover.last_error()
    finally:
        prover.close()
        plus.scratch_trim(0)


# ---- 5. ordering -----------------------------------------------------------------------------------------------------------------------------------------------
def _behind_a_matmul_chain(side, dst, src):
    """dst <- src on `side`, behind a chain of matrix products that keeps the stream busy for milliseconds: a read of dst that is not ordered behind `side` sees
    its old contents.  Nobody synchronises."""
    a = torch.zeros((4096, 4096), device="cuda")
    x = a @ a                              # (the first product loads the BLAS library: not part of the chain)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(24):
            x = x @ a
        dst.copy_(src, non_blocking=True)
    return x


def test_input_produced_on_another_stream():
    kappa, k, b, n = 1, 4, 8, 1 << 15
    m = n // k
    A = lfp.splitmix(40 + kappa, 0, kappa * n * D).reshape(kappa, n, D)
    z = lfp.splitmix(48, 0, m * D).reshape(m, D)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        cm_want = ctx.witness_from_z(z, b, k)
        f_want = ctx.get_witness()
        zd, src = dev(np.zeros((m, D), dtype=np.uint64)), dev(z)
        side = torch.cuda.Stream()
        keep = _behind_a_matmul_chain(side, zd, src)
        cm = hsent(kappa, D)
        assert L().lfplus_ctx_wait_stream(ctx.h, C.c_void_p(side.cuda_stream)) == 0
        assert L().lfplus_witness_from_z_dev(ctx.h, ptr(zd), m, b, k, hp(cm)) == 0
        assert (cm == cm_want).all() and (ctx.get_witness() == f_want).all()
        del keep
    finally:
        ctx.close()


def test_prover_input_produced_on_another_stream():
    A, r1cs, params = _shape(1, 4)
    z = _zs(4, (1,))[0][0]
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    ref = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        cm_want = ref.ingest([z], r1cs)
        flat_want = ref.prove()
        zd, src = dev(np.zeros_like(z)), dev(z)
        side = torch.cuda.Stream()
        keep = _behind_a_matmul_chain(side, zd, src)
        cm = hsent(1, 1, D)
        assert L().lfplus_prover_wait_stream(prover.h, C.c_void_p(side.cuda_stream)) == 0
        assert L().lfplus_prover_ingest_dev(prover.h, (C.c_void_p * 1)(zd.data_ptr()), 1, z.shape[0], 1, hp(cm)) == 0, prover.last_error()
        prover.nfresh = 1
        assert (cm == cm_want).all() and (prover.prove() == flat_want).all()
        del keep
    finally:
        prover.close()
        ref.close()
        plus.scratch_trim(0)


# ---- 6. a pending asynchronous from_f pass is joined before its witness is overwritten ---------------------------------------------------------------------------
def test_device_witnesses_behind_a_pending_async_pass():
    wl = plus.make_plus_workload("P15")
    dp, A = wl.params().lin.decomp, wl.ajtai_matrix()
    z0, z1 = wl.z(0), wl.z(1)
    f0, f1 = plus.gadget_decompose(z0, wl.B, wl.k), plus.gadget_decompose(z1, wl.B, wl.k)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        ctx.set_witness(f0)
        want0 = _rg_read(ctx, dp)
        ctx.set_witness(f1)
        want1 = _rg_read(ctx, dp)
        assert not all((a == b).all() for a, b in zip(want0, want1))
        f0d, z1d = dev(f0), dev(z1)
        ctx.rg_from_f_async(dp)                                               # a pass over f1 in flight ...
        assert L().lfplus_set_witness_dev(ctx.h, ptr(f0d), wl.n) == 0         # ... must be joined before f0 overwrites the witness it reads
        got = _rg_read(ctx, dp)
        assert all((a == b).all() for a, b in zip(got, want0))
        ctx.rg_from_f_async(dp)                                               # the same over f0, then z1 is cut into its place
        cm = hsent(ctx.kappa, D)
        assert L().lfplus_witness_from_z_dev(ctx.h, ptr(z1d), z1.shape[0], wl.B, wl.k, hp(cm)) == 0
        got = _rg_read(ctx, dp)
        assert all((a == b).all() for a, b in zip(got, want1)) and (cm == want1[4]).all()
    finally:
        ctx.close()


# ---- 7. the prover chain, three ways -----------------------------------------------------------------------------------------------------------------------------
def test_prover_chain_from_host_z_device_z_and_device_f():
    """kappa 1, k 4, n = 2^15, rounds (2, 1): NativePlusProver.ingest with host z (the reference: tests/test_gpu_lfplus_native.py pins it to the oracle), ingest with
    device z and accumulator(out=) into device tensors, set_instances with device f and host cm_f -- identical flat proofs, cm_f, accumulators and closing
    challenge; lfplus_verify accepts every proof"""
    kappa, k, rounds = 1, 4, (2, 1)
    A, r1cs, params = _shape(kappa, k)
    zs_all = _zs(k, rounds)

    def chain(way, cms_in=None):
        prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
        ver = plus.NativePlusVerifier.init(A, list(r1cs), params, plus.PoseidonTranscript())
        try:
            out, nacc = [], 0
            for rnd, zs in enumerate(zs_all):
                if way == "host z":
                    cm = prover.ingest(zs, r1cs)
                elif way == "device z":
                    zd = [dev(z) for z in zs]
                    cm = prover.ingest(zd, r1cs)
                    assert all((host(t) == z).all() for t, z in zip(zd, zs))
                else:
                    fd = [dev(plus.gadget_decompose(z, params.B, k)) for z in zs]
                    cm = cms_in[rnd]
                    prover.set_instances(fd, list(cm))
                    for t in fd:
                        t.zero_()                  # (not borrowed: the caller may reuse f as soon as set_instances has returned)
                    torch.cuda.synchronize()
                flat = prover.prove()
                assert ver.verify(flat, nacc + len(zs), len(zs)), (way, ver.stage)
                if way == "device z":
                    acc = tuple(host(t) for t in prover.accumulator(out=(dsent(N, D), dsent(N, D))))
                else:
                    acc = prover.accumulator()
                out.append((flat, cm, acc))
                nacc = 2
            return out, prover.transcript.get_challenge()
        finally:
            prover.close()
    try:
        ref, ref_ch = chain("host z")
        for way in ("device z", "device f"):
            got, ch = chain(way, [cm for _, cm, _ in ref])
            assert ch == ref_ch, way
            for (fa, ca, aa), (fb, cb, ab) in zip(ref, got):
                assert fa.shape == fb.shape and (fa == fb).all(), (way, "proof")
                assert (ca == cb).all(), (way, "cm_f")
                assert (aa[0] == ab[0]).all() and (aa[1] == ab[1]).all(), (way, "accumulator")
    finally:
        plus.scratch_trim(0)
