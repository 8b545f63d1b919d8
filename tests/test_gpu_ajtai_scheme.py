"""AjtaiCommitmentScheme::{commit_coeff, decompose_and_commit_coeff, decompose_and_commit_ntt} (commitment/commitment_scheme.rs:81-113) on the device
against the oracle composed from its existing pieces -- ajtai_commit(A, crt(decompose(f_coeff, B, L, layout 0))) -- and against the resident witness path
(Witness::from_w_ccs + Witness::commit): every digit-plane count the base rule yields on both rings (1 .. 10 Goldilocks, 1 .. 5 BabyBear), digit counts
1 .. 5 over ragged widths (tiles of 8 columns that mix elements), edge coefficients under both digit modes, row chunks, batches, a column chunk longer than the
accumulator flush period, the external basis, the errors, and a sharded context whose rank boundary splits an element's digits."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from latticefold_amd import api
from latticefold_amd.workload import RINGS, make_workload, splitmix_fq

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BASES = {"goldilocks": [2, 2**8, 2**15, 2**16, 2**22, 2**31, 2**32, 2**40, 2**48, 2**50, 2**56, 2**63],     # 1, 2, 3, 3, 4, 5, 5, 6, 7, 8, 9, 10 planes
         "babybear": [2, 2**8, 2**15, 2**16, 2**22, 2**31, 2**32]}                                           # 1, 2, 3, 3, 4, 5, 5


def _oracle(ring):
    if ring == "goldilocks":
        import lfo as O
    else:
        import lfo_bb as O
    return O


def _ctx(ring, env=None):
    os.environ.pop("LF_I8G_WGS", None)
    for k, v in (env or {}).items():
        os.environ[k] = v
    return api.Context(0, ring=ring)


def _rnd(seed, ring, *shape):
    n = int(np.prod(shape))
    return splitmix_fq(seed, 0, n, ring).reshape(shape).copy()


def _coeffs(ring, B, L, count, seed):
    """count elements in coefficient form: the edge residues of the digit rules for base B and L digits, then random ones"""
    p, d, _ = RINGS[ring]
    h = B // 2
    geo = (B**L - 1) // (B - 1)
    edge = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2, h, -h, h - 1, -(h - 1), h + 1, -(h + 1), B**L - 1, -(B**L - 1), B**L, B**L + h,
            h * geo, -h * geo, (h - 1) * geo, -(h + 1) * geo, B**(L - 1) * h, 2**62, 2**62 + 1, -(2**62), p - 2**62 - 1]
    e = np.array([v % p for v in edge], dtype=np.uint64)
    x = _rnd(seed, ring, count, d)
    k = np.arange(count * d)
    flat = x.reshape(-1)
    pick = (k * 7 + k // 5) % (2 * len(e))
    flat[pick < len(e)] = e[pick[pick < len(e)]]                # about half of the coefficients are edge residues
    return x


def _want_dec(O, A, kappa, f_coeff, B, L):
    count = f_coeff.shape[0]
    return O.ajtai_commit(A, kappa, count * L, O.crt(O.decompose(f_coeff, B, L, 0)))


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_every_plane_count_digit_count_and_digit_mode(ring):
    O = _oracle(ring)
    ctx = _ctx(ring)
    kappa = 3 if ring == "goldilocks" else 4
    count = 13                                                  # widths 13, 26, 39, 52, 65: no multiple of 8
    try:
        for L in (1, 2, 3, 4, 5):
            A = _rnd(10 + L, ring, kappa, count * L, ctx.RE)
            scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
            for mode in (0, 1):
                ctx.set_digit_mode(mode)
                O.set_digit_mode(mode)
                for B in BASES[ring]:
                    f = _coeffs(ring, B, L, count, 100 * L + B.bit_length())
                    want = _want_dec(O, A, kappa, f, B, L)
                    assert (scheme.decompose_and_commit_coeff(f, B, L) == want).all(), (L, mode, B)
                    assert (scheme.decompose_and_commit_ntt(O.crt(f), B, L) == want).all(), (L, mode, B)
            if L == 1:
                f = _coeffs(ring, 2**63, 1, count, 5)
                assert (scheme.commit_coeff(f) == O.ajtai_commit(A, kappa, count, O.crt(f))).all()
    finally:
        ctx.set_digit_mode(0)
        O.set_digit_mode(0)
        ctx.close()


@pytest.mark.parametrize("ring,kappa", [("goldilocks", 3), ("goldilocks", 26), ("goldilocks", 99), ("babybear", 4), ("babybear", 16), ("babybear", 21)])
def test_row_chunks_and_batches(ring, kappa):
    O = _oracle(ring)
    ctx = _ctx(ring)
    try:
        count, L, B = 111, 3, 2**16
        A = _rnd(kappa, ring, kappa, count * L, ctx.RE)
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        fs = np.stack([_coeffs(ring, B, L, count, s) for s in (1, 2, 3)])
        want = np.stack([_want_dec(O, A, kappa, f, B, L) for f in fs])
        assert (scheme.decompose_and_commit_coeff(fs, B, L) == want).all()
        assert (scheme.decompose_and_commit_ntt(np.stack([O.crt(f) for f in fs]), B, L) == want).all()
        g = np.stack([_rnd(40 + s, ring, count * L, ctx.RE) for s in (1, 2)])
        assert (scheme.commit_coeff(g) == np.stack([O.ajtai_commit(A, kappa, count * L, O.crt(x)) for x in g])).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_accumulator_flush(ring):
    """two workgroups per row half: 1 400 tiles -> 700 per chunk, longer than the flush period (682 Goldilocks / 227 BabyBear tiles)"""
    O = _oracle(ring)
    ctx = _ctx(ring, {"LF_I8G_WGS": "4" if ring == "goldilocks" else "2"})
    try:
        kappa, count, L, B = (26 if ring == "goldilocks" else 16), 3733, 3, 2**22
        A = _rnd(77, ring, kappa, count * L, ctx.RE)
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        f = _coeffs(ring, B, L, count, 9)
        assert (scheme.decompose_and_commit_coeff(f, B, L) == _want_dec(O, A, kappa, f, B, L)).all()
    finally:
        os.environ.pop("LF_I8G_WGS", None)
        ctx.close()


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_errors_leave_the_context_usable(ring):
    O = _oracle(ring)
    ctx = _ctx(ring)
    try:
        Lib = api._lib()
        f = _coeffs(ring, 2**8, 2, 20, 3)
        out = np.zeros((1, 4, ctx.RE), dtype=np.uint64)
        p_f, p_o = f.ctypes.data_as(api.u64p), out.ctypes.data_as(api.u64p)
        assert Lib.lf_ajtai_decompose_and_commit_coeff(ctx.h, p_f, 20, 2**8, 2, 1, p_o) == -7          # no matrix: LF_ERR_STATE
        A = _rnd(5, ring, 4, 40, ctx.RE)
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        with pytest.raises(api.CommitmentError):
            scheme.decompose_and_commit_coeff(f, 2**8, 3)          # 60 columns for a width of 40
        with pytest.raises(api.CommitmentError):
            scheme.decompose_and_commit_ntt(f[:19], 2**8, 2)
        with pytest.raises(api.CommitmentError):
            scheme.commit_coeff(f)
        assert Lib.lf_ajtai_decompose_and_commit_coeff(ctx.h, p_f, 20, 100, 2, 1, p_o) == -3           # not a power of two: LF_ERR_UNSUPPORTED
        assert Lib.lf_ajtai_decompose_and_commit_ntt(ctx.h, p_f, 20, 0, 2, 1, p_o) == -3
        assert Lib.lf_ajtai_decompose_and_commit_coeff(ctx.h, p_f, 20, 2**8, 0, 1, p_o) == -1           # digits 0: LF_ERR_INVALID
        assert Lib.lf_ajtai_decompose_and_commit_coeff(ctx.h, p_f, 20, 2**8, 2, 0, p_o) == -1           # batch 0
        if ring == "babybear":
            assert Lib.lf_ajtai_decompose_and_commit_coeff(ctx.h, p_f, 20, 2**40, 2, 1, p_o) == -3
        assert (scheme.decompose_and_commit_coeff(f, 2**8, 2) == _want_dec(O, A, 4, f, 2**8, 2)).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_external_basis(ring):
    from test_gpu_ext_basis import general_data, random_T, tower_T
    O = _oracle(ring)
    nonres, y = O.get_ring()
    T = random_T(ring, 4242) if ring == "goldilocks" else tower_T()
    crt, tensor = general_data(ring, nonres, y, T)
    ctx = _ctx(ring)
    try:
        assert O.set_ring_general(crt, tensor) == 0
        ctx.set_ext_basis(T)
        count, L, B, kappa = 29, 3, 2**16, 5
        A = _rnd(31, ring, kappa, count * L, ctx.RE)            # NTT form in the caller's basis
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        f = _coeffs(ring, B, L, count, 8)                       # coefficient form: no basis
        want = _want_dec(O, A, kappa, f, B, L)
        assert (scheme.decompose_and_commit_coeff(f, B, L) == want).all()
        assert (scheme.decompose_and_commit_ntt(O.crt(f), B, L) == want).all()
        g = _rnd(32, ring, count * L, ctx.RE)
        assert (scheme.commit_coeff(g) == O.ajtai_commit(A, kappa, count * L, O.crt(g))).all()
    finally:
        O.set_ring(nonres, y)
        ctx.close()


@pytest.mark.parametrize("name", ["T10", "G5", "E22", "BDP", "B8", "C4"])
def test_equals_the_resident_witness_commitment(name):
    """decompose_and_commit_ntt(w_ccs, B, L) is Witness::from_w_ccs(w_ccs).commit(scheme); commit_coeff(f) is commit_ntt(CRT f) -- C4: 2^18 x 4 columns, kappa 26"""
    wl = make_workload(name)
    ctx = _ctx(wl.ring)
    try:
        ctx.load_ccs(wl)
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        want = wit.commit(scheme)
        assert (scheme.decompose_and_commit_ntt(wl.w_ccs, wl.B, wl.L) == want).all()
        f = wit.f_coeff
        assert (scheme.decompose_and_commit_coeff(ctx.icrt(wl.w_ccs), wl.B, wl.L) == want).all()
        assert (scheme.commit_coeff(f) == want).all()
        g = _rnd(3, wl.ring, wl.N, ctx.RE)
        assert (scheme.commit_coeff(g) == scheme.commit_ntt(ctx.crt(g))).all()
    finally:
        ctx.close()


WORKER = textwrap.dedent('''
    import os, sys, json
    sys.path.insert(0, os.environ["LF_ROOT"]); sys.path.insert(0, os.path.join(os.environ["LF_ROOT"], "tests"))
    import numpy as np, torch.distributed as dist
    from latticefold_amd import api, dist as lfd
    from latticefold_amd.workload import splitmix_fq
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    out = {}
    for ring, count, L, B in (("goldilocks", 333, 4, 2**16), ("goldilocks", 111, 6, 2**8), ("babybear", 333, 4, 2**22)):
        d = 24 if ring == "goldilocks" else 72
        A = splitmix_fq(1, 0, 7 * count * L * d, ring).reshape(7, count * L, d)
        f = splitmix_fq(2, 0, 2 * count * d, ring).reshape(2, count, d)
        g = splitmix_fq(3, 0, count * L * d, ring).reshape(count * L, d)
        def run(sharded):
            ctx = api.Context(0, ring=ring)
            if sharded:
                lfd.init_sharding(ctx, rank, world, "host")
            s = api.AjtaiCommitmentScheme(ctx, matrix=A)
            w = np.stack([ctx.crt(x) for x in f])
            r = [s.decompose_and_commit_coeff(f, B, L), s.decompose_and_commit_ntt(w, B, L), s.commit_coeff(g)]
            ctx.close()
            return [x.tolist() for x in r]
        ref = run(False)
        got = run(True)
        out["%s/%d/%d" % (ring, count, L)] = got == ref
    allg = [None] * world
    dist.all_gather_object(allg, out)
    if rank == 0:
        print(json.dumps(allg))
    dist.destroy_process_group()
''')


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_rank_boundary_inside_an_element(tmp_path):
    """two ranks on one GPU over the host transport; widths 1332 = 2 x 666 (L 4: the boundary falls after digit 2 of element 166) and 666 = 2 x 333 (L 6:
    after digit 3 of element 55): every rank returns the unsharded commitment"""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, LF_ROOT=ROOT, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    ranks = json.loads([l for l in out.stdout.splitlines() if l.startswith("[")][-1])
    assert len(ranks) == 2 and all(len(r) == 3 and all(r.values()) for r in ranks), ranks
