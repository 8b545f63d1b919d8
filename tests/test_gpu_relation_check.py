"""Relation checks on the device, both rings: CCS::check_relation (arith.rs:76-110) through lf_ccs_check -- satisfied systems of every shape, the exact first
bad row against the host restatement of tests/test_relation_check_cpu.py --, R_CCCS (lf_cccs_check) and the decider of an accumulator, R_LCCCS (lf_lcccs_check,
arith.rs:193-206), on linearized instances, fold-step outputs and the end of a chain; an external basis; the error codes."""
import numpy as np
import pytest

from latticefold_amd import api
from latticefold_amd.workload import RINGS, chain_w_ccs, diag, make_workload, splitmix_fq
from test_relation_check_cpu import bad_rows, residual_host

pytestmark = pytest.mark.gpu


def ctx_for(wl):
    ctx = api.Context(0, ring=wl.ring)
    ctx.load_ccs(wl)
    return ctx


def host_first_bad(wl, z):
    rows = bad_rows(residual_host(wl, z))
    return int(rows[0]) if len(rows) else wl.m


def device_first_bad(ctx, z):
    try:
        ctx.check_relation(z)
        return ctx.m
    except api.NotSatisfied as e:
        return e.row


def tr(wl):
    return api.PoseidonTranscript(ring=wl.ring)


def lcccs_rows(wl):
    """first row of r, v, cm, u, x_w, h in a flat LCCCS"""
    r = 0
    v = r + wl.s
    cm = v + wl.tau
    u = cm + wl.kappa
    x = u + wl.t
    return {"r": r, "v": v, "cm": cm, "u": u, "x": x, "h": x + wl.l}


def bump(a, row, word, P):
    a = a.copy()
    a[row, word] = (int(a[row, word]) + 1) % P
    return a


@pytest.mark.parametrize("name", ["T10", "T14", "B8", "B14"])
def test_satisfied_systems_pass(name):
    for ccs in ("r1cs", "multi4", "multi16", "deg3"):
        wl = make_workload(name, ccs=ccs)
        ctx = ctx_for(wl)
        try:
            assert ctx.check_relation(wl.z()) is None, ccs
        finally:
            ctx.close()


def test_satisfied_at_c2():
    wl = make_workload("C2")
    ctx = ctx_for(wl)
    try:
        assert ctx.check_relation(wl.z()) is None
    finally:
        ctx.close()


@pytest.mark.parametrize("name,ccs", [("T10", "r1cs"), ("T10", "multi4"), ("B8", "r1cs"), ("B8", "multi16")])
def test_first_bad_row_matches_the_host(name, ccs):
    wl = make_workload(name, ccs=ccs)
    ctx = ctx_for(wl)
    try:
        base = wl.l + 1
        z = wl.z()
        # one tampered witness element
        z1 = bump(z, base + 11, 0, wl.P)
        assert device_first_bad(ctx, z1) == host_first_bad(wl, z1) < wl.m
        # several bad rows: the smallest wins
        zs = z.copy()
        for c in (base + 100, base + 20, base + 60):
            zs = bump(zs, c, 5, wl.P)
        want = host_first_bad(wl, zs)
        assert device_first_bad(ctx, zs) == want < wl.m
        # a tampered matrix value (matrix 2, an entry of row 30)
        k = int(np.asarray(wl.rowptr[2])[30])
        wl.val[2] = np.ascontiguousarray(wl.val[2]).copy()
        wl.val[2][k, 1] = (int(wl.val[2][k, 1]) + 3) % wl.P
        ctx.load_ccs(wl)
        want = host_first_bad(wl, z)
        assert want <= 30 and device_first_bad(ctx, z) == want
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["T10", "B8"])
def test_last_row_behind_empty_rows_and_single_words(name):
    """m > n: rows n .. m-1 are empty.  Matrix C gets one entry in row m-1 at the constant column (z_l = 1), so the residual of that row is -value: all
    words (value 1), or exactly ONE word of one slot"""
    wl0 = make_workload(name)
    assert wl0.m > wl0.n
    p, d, tau = RINGS[wl0.ring]
    values = [diag(1, wl0.ring)]
    for w in (0, d - 1, 3 * tau + 1):
        e = np.zeros(d, dtype=np.uint64)
        e[w] = 1
        values.append(e)
    ctx = api.Context(0, ring=wl0.ring)
    try:
        for val in values:
            wl = make_workload(name)
            rp = np.asarray(wl.rowptr[2]).astype(np.uint32).copy()
            rp[wl.m] += 1
            wl.rowptr[2] = rp
            wl.col[2] = np.append(np.asarray(wl.col[2]), np.uint32(wl.l)).astype(np.uint32)
            wl.val[2] = np.concatenate([np.asarray(wl.val[2]), val[None, :]]).astype(np.uint64)
            ctx.load_ccs(wl)
            z = wl.z()
            assert host_first_bad(wl, z) == wl.m - 1
            assert device_first_bad(ctx, z) == wl.m - 1, val.nonzero()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["T10", "B8"])
def test_cccs(name):
    wl = make_workload(name)
    ctx = ctx_for(wl)
    try:
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        assert ctx.check_cccs(cccs, wit) == set() and ctx.last_first_bad == wl.m
        _ok, norm = ctx.linf_check(wit.f, wl.B)
        assert ctx.check_cccs(cccs, wit, bound=norm + 1) == set()
        assert ctx.check_cccs(cccs, wit, bound=norm) == {"norm"}
        assert ctx.check_cccs(bump(cccs, 1, 7, wl.P), wit) == {"cm"}
        x2 = bump(cccs, wl.kappa, 0, wl.P)
        assert ctx.check_cccs(x2, wit) == {"ccs"}
        z2 = np.concatenate([x2[wl.kappa:], diag(1, wl.ring)[None, :], wl.w_ccs])
        assert ctx.last_first_bad == host_first_bad(wl, z2) < wl.m
        assert ctx.check_cccs(bump(x2, 0, 0, wl.P), wit, bound=norm) == {"cm", "ccs", "norm"}
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["T10", "B8", "C2"])
def test_lcccs_decider(name):
    wl = make_workload(name)
    ctx = ctx_for(wl)
    try:
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr(wl))
        assert ctx.check_lcccs(acc, wit) == set()
        assert ctx.check_lcccs(acc, wit, bound=wl.B) == set()
        lc, w1, _ = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr(wl))
        assert ctx.check_lcccs(lc, w1, bound=wl.B) == set()
        R = lcccs_rows(wl)
        assert ctx.check_lcccs(bump(lc, R["u"] + wl.t - 1, 3, wl.P), w1) == {"u"}
        assert ctx.check_lcccs(bump(lc, R["v"] + 1, 4, wl.P), w1) == {"v"}
        assert ctx.check_lcccs(bump(lc, R["cm"] + 2, 0, wl.P), w1) == {"cm"}
        h2 = lc.copy()
        h2[R["h"]] = diag(2, wl.ring)
        assert ctx.check_lcccs(h2, w1) == {"u"}
        _ok, norm = ctx.linf_check(w1.f, wl.B)
        assert ctx.check_lcccs(lc, w1, bound=norm) == {"norm"}
        # the witness of another step
        other = api.Witness.from_w_ccs(ctx, chain_w_ccs(wl, 1))
        assert ctx.check_lcccs(lc, other) == {"cm", "u", "v"}
        assert ctx.check_lcccs(acc, other) == {"cm", "u", "v"}
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["T10", "B8"])
def test_chain_accumulator_decides(name):
    wl = make_workload(name)
    ctx = ctx_for(wl)
    try:
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        w_acc = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        acc, _ = api.LFLinearizationProver.prove(ctx, np.concatenate([w_acc.commit(scheme), wl.x_ccs]), w_acc, tr(wl))
        for j in (1, 2, 3):
            w_j = api.Witness.from_w_ccs(ctx, chain_w_ccs(wl, j))
            cccs = np.concatenate([w_j.commit(scheme), wl.x_ccs])
            assert ctx.check_cccs(cccs, w_j, bound=wl.B // 2 + 1) == set()
            acc, w_acc, _ = api.NIFSProver.prove(ctx, acc, w_acc, cccs, w_j, tr(wl))
        assert ctx.check_lcccs(acc, w_acc, bound=wl.B) == set()
    finally:
        ctx.close()


def random_T(ring, seed):
    """an invertible basis change of F_{p^tau} that fixes 1 (as tests/test_gpu_ext_basis.py)"""
    p, _d, tau = RINGS[ring]
    while True:
        T = splitmix_fq(seed, 0, tau * tau, ring).reshape(tau, tau).copy()
        T[:, 0] = 0
        T[0, 0] = 1
        M = [[int(v) % p for v in row] for row in T]
        ok = True
        for c in range(tau):    # Gaussian elimination: singular -> next seed
            piv = next((r for r in range(c, tau) if M[r][c]), None)
            if piv is None:
                ok = False
                break
            M[c], M[piv] = M[piv], M[c]
            iv = pow(M[c][c], p - 2, p)
            for r in range(c + 1, tau):
                f = M[r][c] * iv % p
                M[r] = [(a - f * b) % p for a, b in zip(M[r], M[c])]
        if ok:
            return T
        seed += 1


@pytest.mark.parametrize("name", ["T8", "B6"])
def test_external_basis(name):
    wl = make_workload(name)
    ctx = api.Context(0, ring=wl.ring)
    try:
        ctx.set_ext_basis(random_T(wl.ring, 4242))
        ctx.load_ccs(wl)
        assert ctx.check_relation(wl.z()) is None
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        assert ctx.check_cccs(cccs, wit) == set()
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr(wl))
        lc, w1, _ = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr(wl))
        assert ctx.check_lcccs(acc, wit) == set()
        assert ctx.check_lcccs(lc, w1, bound=wl.B) == set()
        assert ctx.check_lcccs(bump(lc, lcccs_rows(wl)["v"], 1, wl.P), w1) == {"v"}
    finally:
        ctx.close()


def test_error_codes():
    wl = make_workload("T10")
    bare = api.Context(0)
    try:
        with pytest.raises(api.LfError) as e:
            bare.check_relation(wl.z())
        assert e.value.code == -7                     # no CCS: LF_ERR_STATE
        bare.load_ccs(wl)
        wit0 = api.Witness.from_w_ccs(bare, wl.w_ccs)
        with pytest.raises(api.LfError) as e:
            bare.check_cccs(np.concatenate([np.zeros((wl.kappa, 24), np.uint64), wl.x_ccs]), wit0)
        assert e.value.code == -7                     # no Ajtai matrix: LF_ERR_STATE
    finally:
        bare.close()
    ctx, other = ctx_for(wl), ctx_for(wl)
    try:
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr(wl))
        foreign = api.Witness.from_w_ccs(other, wl.w_ccs)
        for call in (lambda: ctx.check_cccs(cccs, foreign), lambda: ctx.check_lcccs(acc, foreign)):
            with pytest.raises(api.LfError) as e:
                call()
            assert e.value.code == -1                 # a witness of another context: LF_ERR_INVALID
        nd = acc.copy()
        nd[0, 3] = (int(nd[0, 3]) + 1) % wl.P          # slot 1 of r_0 differs from slot 0: not a diagonal challenge
        with pytest.raises(api.LfError) as e:
            ctx.check_lcccs(nd, wit)
        assert e.value.code == -3                     # LF_ERR_UNSUPPORTED
    finally:
        ctx.close()
        other.close()
    sh = api.Context(0)
    try:
        sh.set_sharding_model(0, 2)
        sh.load_ccs(wl)
        with pytest.raises(api.LfError) as e:
            sh.check_relation(wl.z())
        assert e.value.code == -3                     # sharded: LF_ERR_UNSUPPORTED
    finally:
        sh.close()
