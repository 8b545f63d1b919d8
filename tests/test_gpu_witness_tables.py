"""The witness tables of include/lfhip_tables.h on the device, both spellings (host arrays and the caller's device memory), against the numpy restatements of
tests/witness_tables_ref.py (which tests/test_witness_tables_cpu.py holds to the CPU oracle) and against the library's own neighbours:

  lf_witness_get_fhat   word for word against the formula; its tables evaluate to v of lf_linearize; 2K part handles in one call feed lf_sumcheck_fold_begin_dev
  lf_witness_get_z/_mz  against wl.z() and lf_spmv per matrix; the device tables drive lf_mlsumcheck_prove_device
  lf_spmv_t             against a scatter-add over the entries, on the workloads' matrices and on hand-built ones around the heavy-column path's constants
  lf_mle_fix_variables  against the numpy fix; nfix = nv is lf_mle_eval_batch
  all of them in an external basis, their refusals, and a fold step next to them."""
import ctypes as C

import numpy as np
import pytest
import torch

from latticefold_amd import api
from latticefold_amd.workload import RINGS, make_workload
from witness_parts_cases import oracle_parts, residues
from witness_tables_ref import (SPMV_T_CHUNK, SPMV_T_HEAVY, csr_from_columns, embed, fhat_np, fix_np, inner_np, lcccs_parts, oracle_for, rand_ring, spmv_t_np,
                                workload)

pytestmark = pytest.mark.gpu

INVALID, HIP, UNSUPPORTED, STATE = -1, -2, -3, -7
PATTERN = -0x5A5A5A5A5A5A5A5B


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def filled(shape):
    return torch.full(shape, PATTERN, dtype=torch.int64, device="cuda")


class Case:
    """a context with the workload's constraint system and Ajtai matrix, its witness and its linearized instance"""

    def __init__(self, wl, ajtai=True):
        self.wl = wl
        self.ctx = api.Context(0, ring=wl.ring)
        self.ctx.load_ccs(wl)
        self.scheme = api.AjtaiCommitmentScheme(self.ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed()) if ajtai else None
        self.wit = api.Witness.from_w_ccs(self.ctx, wl.w_ccs)

    def tr(self):
        return api.PoseidonTranscript(ring=self.wl.ring)

    def linearize(self):
        self.cccs = np.concatenate([self.wit.commit(self.scheme), self.wl.x_ccs])
        acc, _ = api.LFLinearizationProver.prove(self.ctx, self.cccs, self.wit, self.tr())
        self.acc = acc
        return lcccs_parts(acc, self.wl)

    def close(self):
        self.ctx.close()


# ---- 1. f-hat ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T8", "G5", "R61b4", "B6", "BDP", "B333"])
def test_fhat_is_the_formula_and_evaluates_to_v(name):
    wl = make_workload(name, 0)
    case = Case(wl)
    try:
        ctx, wit = case.ctx, case.wit
        want = fhat_np(wit.f_coeff, wl)
        assert (wit.get_fhat() == want).all()
        got = wit.get_fhat(device=True)
        assert tuple(got.shape) == (wl.tau, wl.m, wl.RE) and (host(got) == want).all()
        flat = filled((wl.tau * wl.m * wl.RE + 1,))          # an output that is 8- but not 16-byte aligned: the kernel's one-word stores
        odd = wit.get_fhat(device=flat[1:].view(wl.tau, wl.m, wl.RE))
        assert odd.data_ptr() % 16 == 8 and (host(odd) == want).all() and int(flat[0]) == PATTERN
        # coefficients at +-(B/2 - 1), 0 and +-1 in known positions: every value in every one of the RE coefficient positions (every slot of every table)
        edge = np.array([wl.B // 2 - 1, -(wl.B // 2 - 1), 0, 1, -1], dtype=np.int64)
        i, c = np.meshgrid(np.arange(wl.N), np.arange(wl.RE), indexing="ij")
        f = residues(edge[(i + c) % 5], wl.P)
        w2 = api.Witness.from_f_coeff(ctx, f)
        want2 = fhat_np(f, wl)
        assert (w2.get_fhat() == want2).all()
        both = api.get_fhat(ctx, [wit, w2], device=filled((2 * wl.tau, wl.m, wl.RE)))    # two witnesses, one call, table w tau + j
        assert (host(both) == np.concatenate([want, want2])).all()
        assert (api.get_fhat(ctx, [w2, wit]) == np.concatenate([want2, want])).all()
        r, v, _ = case.linearize()
        assert (ctx.evaluate_mles(got, r[:, :wl.tau]) == v).all()
    finally:
        case.close()


# ---- 2. the fold sumcheck from device-built tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T8", "B6"])
def test_fold_sumcheck_from_device_built_fhat(name):
    wl = make_workload(name, 0)
    O = oracle_for(wl.ring)
    case = Case(wl, ajtai=False)
    try:
        ctx, m, tau, K2 = case.ctx, wl.m, wl.tau, 2 * wl.K
        parts = case.wit.decompose(ctx) + case.wit.decompose(ctx)                       # 2K handles
        tables = filled((5 + K2 * tau, m, wl.RE))
        head = rand_ring(77, 5 * m, wl).reshape(5, m, wl.RE)
        for idx, sd in ((0, 1), (2, 2), (4, 3)):
            head[idx] = O.build_eq(np.stack([embed(c) for c in rand_ring(100 + sd, wl.s, wl)[:, :tau]]))
        tables[:5] = dev(head)
        api.get_fhat(ctx, parts, device=tables[5:])                                     # all 2K in one call, into slots 5..
        ref = oracle_parts(O, wl, O.Instance(wl).witness_from_w_ccs(wl.w_ccs), 0)
        tab_np = np.concatenate([head] + [fhat_np(ref[k % wl.K], wl) for k in range(K2)])
        assert (host(tables) == tab_np).all()
        mu = rand_ring(9, K2, wl)[:, :tau].copy()
        msgs_o, pt_o = O.Instance(wl).sumcheck_fold(O.Transcript(), tab_np, np.stack([embed(c) for c in mu]))
        sc = api.MLSumcheckFold(ctx, tables, mu)
        npts = 2 * wl.b + 1
        for rnd in range(wl.s):
            ev = sc.prove_round(None if rnd == 0 else pt_o[rnd - 1][:tau])
            assert (ev == msgs_o[rnd * npts:(rnd + 1) * npts]).all(), f"round {rnd + 1}"
        sc.end()
    finally:
        case.close()


# ---- 3. z and M z --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ccs,l", [("T8", "r1cs", 1), ("T12", "general5", 1), ("T10", "mix8", 2), ("B6", "multi", 1), ("T8b4", "r1cs", 1)])
def test_z_and_mz_and_the_generic_sumcheck_on_them(name, ccs, l):
    wl = workload(name, ccs, l)
    O = oracle_for(wl.ring)
    case = Case(wl, ajtai=False)
    try:
        ctx, wit, z = case.ctx, case.wit, wl.z()
        assert (wit.get_z(wl.x_ccs) == z).all()
        zd = wit.get_z(wl.x_ccs, device=True)
        assert (host(zd) == z).all()
        want = np.stack([ctx.mat_vec_mul(j, z) for j in range(wl.t)])
        assert (wit.mz(wl.x_ccs) == want).all()
        tabs = filled((wl.t + 1, wl.m, wl.RE))
        wit.mz(wl.x_ccs, device=tabs[:wl.t])
        assert (host(tabs[:wl.t]) == want).all()
        # the CCS's own product list times eq: sum_i c_i prod_{j in S_i} (M_j z) eq, on the device tables and on the same tables from the host
        eq = O.build_eq(np.stack([embed(c) for c in rand_ring(31, wl.s, wl)[:, :wl.tau]]))
        tabs[wl.t] = dev(eq)
        terms = [(wl.c[i], [int(j) for j in wl.S_idx[wl.S_off[i]:wl.S_off[i + 1]]] + [wl.t]) for i in range(wl.q)]
        vp = api.VPoly(terms)
        msgs_d, pt_d, fin_d = api.MLSumcheck.prove(ctx, case.tr(), tabs, vp)
        msgs_h, pt_h, fin_h = api.MLSumcheck.prove(ctx, case.tr(), np.concatenate([want, eq[None]]), vp)
        assert (msgs_d == msgs_h).all() and (pt_d == pt_h).all() and (fin_d == fin_h).all()
    finally:
        case.close()


# ---- 4. M^T v ------------------------------------------------------------------------------------------------------------------------------------------
def _check_spmv_t(ctx, wl, j, v, tag):
    want = spmv_t_np(wl.rowptr[j], wl.col[j], wl.val[j], v, wl.n, wl.ring)
    assert (ctx.mat_vec_mul_t(j, v) == want).all(), (tag, j, "host")
    got = ctx.mat_vec_mul_t(j, dev(v), out=filled((wl.n, wl.RE)))
    assert (host(got) == want).all(), (tag, j, "device")
    assert (host(ctx.mat_vec_mul_t(j, v, device=True)) == want).all(), (tag, j, "uploaded")
    return got


@pytest.mark.parametrize("name,ccs", [("T8", "r1cs"), ("T10", "multi16"), ("T12", "general5"), ("B6", "multi"), ("B333", "r1cs")])
def test_spmv_t_on_the_workloads_matrices(name, ccs):
    wl = workload(name, ccs)
    case = Case(wl, ajtai=False)
    try:
        ctx = case.ctx
        assert ctx.spmv_t_heavy_min() == SPMV_T_HEAVY
        v, z = rand_ring(41, wl.m, wl), wl.z()
        for j in range(wl.t):
            out = _check_spmv_t(ctx, wl, j, v, name)
            # <M z, v> = <z, M^T v> through lf_ring_mul_device, n_terms = m and n
            lhs = ctx.ring_mul(ctx.mat_vec_mul(j, dev(z)).reshape(wl.m, 1, wl.RE), dev(v).reshape(wl.m, 1, wl.RE))
            rhs = ctx.ring_mul(dev(z).reshape(wl.n, 1, wl.RE), out.reshape(wl.n, 1, wl.RE))
            assert (host(lhs) == host(rhs)).all(), (name, j)
    finally:
        case.close()


@pytest.mark.parametrize("name", ["T8", "B6"])
def test_spmv_t_of_eq_is_what_the_prover_computes(name):
    """v = the ring-element form of eq(r): <z, M_j^T eq(r)> = u_j of lf_linearize"""
    wl = make_workload(name, 0)
    O = oracle_for(wl.ring)
    case = Case(wl)
    try:
        r, _, u = case.linearize()
        eq, z = O.build_eq(r), wl.z()
        for j in range(wl.t):
            assert (inner_np(z, case.ctx.mat_vec_mul_t(j, eq), wl.ring) == u[j]).all(), (name, j)
    finally:
        case.close()


def _hand_built(wl):
    """three matrices at s = 10 around the constants of the heavy-column path: an empty one; one with empty first and last columns, a column holding all
    1024 rows next to a second heavy one, columns of SPMV_T_HEAVY - 1, SPMV_T_HEAVY, SPMV_T_HEAVY + 1 entries, and heavy columns that end just before, at and
    just after a work item (SPMV_T_CHUNK entries); one with heavy columns around the 32-entry stride of a work item's block and the 8 entries of a wave"""
    m, n, T, CH = wl.m, wl.n, SPMV_T_HEAVY, SPMV_T_CHUNK
    assert m == 1024 and n > 64
    a = np.zeros(n, dtype=np.int64)
    b = np.arange(n, dtype=np.int64) % 4
    b[0] = b[n - 1] = 0
    b[5], b[6] = 1024, 700
    b[10:13] = [T - 1, T, T + 1]
    b[20:24] = [CH - 1, CH, CH + 1, 2 * CH - 1]
    b[31:34] = [T + 5, 1, T + 9]                     # heavy columns at the end of one 32-column block and the start of the next
    c = np.arange(n, dtype=np.int64) % 3
    c[40:46] = [T + 31, T + 32, T + 33, T + 7, T + 8, CH + 32]
    c[n - 1] = 1024
    mats = [csr_from_columns(cnt, m, n, wl, 900 + i) for i, cnt in enumerate((a, b, c))]
    for j, (rp, ci, va) in enumerate(mats):
        wl.rowptr[j], wl.col[j], wl.val[j] = rp, ci, (va if len(va) else np.zeros((0, wl.RE), dtype=np.uint64))
    return wl


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_spmv_t_on_hand_built_columns_whatever_path_they_take(ring):
    wl = _hand_built(make_workload("T10", 0))
    if ring == "babybear":                                   # the same shape on the other ring
        bb = make_workload("B6", 0)
        bb.s, bb.wit_len, bb.L = 10, 256, 2
        bb.x_ccs, bb.w_ccs = bb.x_ccs[:1], rand_ring(7, 256, bb)
        bb.rowptr, bb.col, bb.val = [None] * 3, [None] * 3, [None] * 3
        wl = _hand_built(bb)
    v = rand_ring(43, wl.m, wl)
    outs = []
    for heavy_min in (0, 1, 1 << 30):                        # the shipped threshold; every non-empty column heavy; none
        ctx = api.Context(0, ring=wl.ring)
        try:
            ctx.spmv_t_heavy_min(next=heavy_min)
            ctx.load_ccs(wl)
            assert ctx.spmv_t_heavy_min() == (heavy_min or SPMV_T_HEAVY)
            got = [_check_spmv_t(ctx, wl, j, v, (ring, heavy_min)) for j in range(3)]
            outs.append([host(g) for g in got])
            assert not outs[-1][0].any()                     # the empty matrix
            z = rand_ring(44, wl.n, wl)
            for j in range(3):                               # <M z, v> = <z, M^T v> through lf_ring_mul_device, n_terms = m and n
                lhs = ctx.ring_mul(ctx.mat_vec_mul(j, dev(z)).reshape(wl.m, 1, wl.RE), dev(v).reshape(wl.m, 1, wl.RE))
                rhs = ctx.ring_mul(dev(z).reshape(wl.n, 1, wl.RE), got[j].reshape(wl.n, 1, wl.RE))
                assert (host(lhs) == host(rhs)).all(), (ring, heavy_min, j)
        finally:
            ctx.close()
    for o in outs[1:]:
        assert all((a == b).all() for a, b in zip(o, outs[0]))


# ---- 5. fix_variables on tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,nv,ntables", [("goldilocks", nv, nt) for nv in (1, 5, 11) for nt in (1, 3, 7)] + [("babybear", 1, 1), ("babybear", 5, 3), ("babybear", 11, 7)])
def test_mle_fix_variables(ring, nv, ntables):
    wl = make_workload("T8" if ring == "goldilocks" else "B6", 0)
    ctx = api.Context(0, ring=ring)                          # a bare context
    try:
        tabs = rand_ring(1000 * nv + ntables, ntables << nv, wl).reshape(ntables, 1 << nv, wl.RE)
        point = rand_ring(nv + 50, nv, wl)[:, :wl.tau].copy()
        want, cur = {}, tabs
        for i in range(nv):
            cur = fix_np(cur, embed(point[i]), ring)
            want[i + 1] = cur
        td = dev(tabs)
        for nfix in sorted({1, nv - 1, nv} - {0}):
            assert (api.mle_fix_variables(ctx, tabs, point[:nfix]) == want[nfix]).all(), nfix
            got = api.mle_fix_variables(ctx, td, point[:nfix], out=filled((ntables, 1 << (nv - nfix), wl.RE)))
            assert (host(got) == want[nfix]).all(), nfix
        assert (want[nv][:, 0] == ctx.evaluate_mles(tabs, point)).all()
        assert (host(td) == tabs).all()                      # the input tables are read only
    finally:
        ctx.close()


# ---- 6. external basis (Goldilocks) --------------------------------------------------------------------------------------------------------------------
def test_tables_in_an_external_basis():
    from test_gpu_ext_basis import random_T
    wl = make_workload("T8", 0, ccs="multi")
    p, d, tau = RINGS[wl.ring]
    T = random_T(wl.ring, 4242)
    To = T.astype(object)

    def to_ext(a):
        x = np.asarray(a, dtype=np.uint64).astype(object).reshape(-1, tau)
        return ((x @ To.T) % p).astype(np.uint64).reshape(np.shape(a))

    ref = Case(wl, ajtai=False)
    ctx = api.Context(0)
    try:
        ctx.set_ext_basis(T)
        wx = make_workload("T8", 0, ccs="multi")
        wx.val, wx.c, wx.x_ccs, wx.w_ccs = [to_ext(v) for v in wl.val], to_ext(wl.c), to_ext(wl.x_ccs), to_ext(wl.w_ccs)
        ctx.load_ccs(wx)
        wit = api.Witness.from_w_ccs(ctx, wx.w_ccs)
        assert (wit.f_coeff == ref.wit.f_coeff).all()
        fh = ref.wit.get_fhat()
        assert (to_ext(fh) == fh).all()                      # constant slots: the same words in any basis
        assert (wit.get_fhat() == fh).all() and (host(wit.get_fhat(device=True)) == fh).all()
        z = to_ext(ref.wit.get_z(wl.x_ccs))
        assert (wit.get_z(wx.x_ccs) == z).all() and (host(wit.get_z(wx.x_ccs, device=True)) == z).all()
        mz = to_ext(ref.wit.mz(wl.x_ccs))
        assert (wit.mz(wx.x_ccs) == mz).all() and (host(wit.mz(wx.x_ccs, device=True)) == mz).all()
        v = rand_ring(47, wl.m, wl)
        tabs = rand_ring(48, 3 * 32, wl).reshape(3, 32, wl.RE)
        point = rand_ring(49, 5, wl)[:, :tau].copy()
        for j in range(wl.t):
            want = to_ext(ref.ctx.mat_vec_mul_t(j, v))
            assert (ctx.mat_vec_mul_t(j, to_ext(v)) == want).all() and (host(ctx.mat_vec_mul_t(j, dev(to_ext(v)))) == want).all()
        for nfix in (2, 5):
            want = to_ext(api.mle_fix_variables(ref.ctx, tabs, point[:nfix]))
            assert (api.mle_fix_variables(ctx, to_ext(tabs), to_ext(point[:nfix])) == want).all()
            assert (host(api.mle_fix_variables(ctx, dev(to_ext(tabs)), to_ext(point[:nfix]))) == want).all()
    finally:
        ref.close()
        ctx.close()


# ---- 7. refusals, 8. no change next to it --------------------------------------------------------------------------------------------------------------
def _step_equals_oracle(ctx, wl):
    O = oracle_for(wl.ring)
    inst = O.Instance(wl)
    A = inst.ajtai_matrix()
    f = inst.witness_from_w_ccs(wl.w_ccs)
    cccs = np.concatenate([O.ajtai_commit(A, wl.kappa, wl.N, O.crt(f)), wl.x_ccs])
    acc_o, _ = inst.linearize(O.Transcript(), cccs, f)
    lc_o, f0_o, proof_o = inst.fold_step(O.Transcript(), A, acc_o, f, cccs, f)
    api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    tr = lambda: api.PoseidonTranscript(ring=wl.ring)
    acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr())
    lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr())
    assert (acc == acc_o).all() and (lc == lc_o).all() and (proof == proof_o).all() and (w0.f == f0_o).all()


def _rc(fn, *args):
    return int(fn(*args))


def test_refusals_leave_outputs_and_context_alone():
    L = api._lib()
    wl = make_workload("T8", 0)
    u64p, vp = C.POINTER(C.c_uint64), C.c_void_p
    ctx, other, bare, model = api.Context(0), api.Context(0), api.Context(0), api.Context(0)
    try:
        ctx.load_ccs(wl)
        other.load_ccs(wl)
        wit, foreign = api.Witness.from_w_ccs(ctx, wl.w_ccs), api.Witness.from_w_ccs(other, wl.w_ccs)
        m, n, RE, tau, t = wl.m, wl.n, wl.RE, wl.tau, wl.t
        x = np.ascontiguousarray(wl.x_ccs)
        xp = x.ctypes.data_as(u64p)
        hs = lambda *ws: api._handles(list(ws))
        big = filled((max(tau, t) * m + n, RE))                   # every device output below fits; pre-filled with the pattern
        out, hout = vp(big.data_ptr()), np.zeros((max(tau, t) * m + n, RE), dtype=np.uint64)
        hp = hout.ctypes.data_as(u64p)
        v = dev(rand_ring(1, m, wl))
        pt = np.ascontiguousarray(rand_ring(2, 8, wl)[:, :tau])
        ptp = pt.ctypes.data_as(u64p)
        tabs = dev(rand_ring(3, 2 * 64, wl))
        ctx.wait_stream()
        null = None
        vh = rand_ring(1, m, wl)
        want0 = spmv_t_np(wl.rowptr[0], wl.col[0], wl.val[0], vh, n, wl.ring)

        def usable():   # the context still computes, and nothing reached the outputs of the refused calls
            assert (ctx.mat_vec_mul_t(0, vh) == want0).all() and (wit.get_z(x) == wl.z()).all()
            torch.cuda.synchronize()
            assert (big == PATTERN).all() and not hout.any()

        checks = [
            # 1. NULL arguments, a handle of another context
            (INVALID, L.lf_witness_get_fhat_device, (ctx.h, null, 1, out)), (INVALID, L.lf_witness_get_fhat_device, (ctx.h, hs(wit), 1, null)),
            (INVALID, L.lf_witness_get_fhat_device, (ctx.h, hs(foreign), 1, out)), (INVALID, L.lf_witness_get_fhat, (ctx.h, hs(wit, foreign), 2, hp)),
            (INVALID, L.lf_witness_get_z_device, (ctx.h, wit.h, null, out)), (INVALID, L.lf_witness_get_z_device, (ctx.h, foreign.h, xp, out)),
            (INVALID, L.lf_witness_mz_device, (ctx.h, null, xp, out)), (INVALID, L.lf_witness_mz, (ctx.h, wit.h, xp, null)),
            (INVALID, L.lf_spmv_t_device, (ctx.h, 0, null, out)), (INVALID, L.lf_spmv_t_device, (null, 0, vp(v.data_ptr()), out)),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, vp(tabs.data_ptr()), 2, 64, null, 1, out)),
            usable,
            # 2. no constraint system (fix_variables works on a bare context: below)
            (STATE, L.lf_spmv_t_device, (bare.h, 0, vp(v.data_ptr()), out)), (STATE, L.lf_spmv_t, (bare.h, 0, hp, hp)),
            usable,
            # 3. j >= t, count == 0, len not a power of two, nfix outside 1 .. nv
            (INVALID, L.lf_spmv_t_device, (ctx.h, t, vp(v.data_ptr()), out)), (INVALID, L.lf_witness_get_fhat_device, (ctx.h, hs(wit), 0, out)),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, vp(tabs.data_ptr()), 2, 48, ptp, 1, out)),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, vp(tabs.data_ptr()), 2, 64, ptp, 0, out)),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, vp(tabs.data_ptr()), 2, 64, ptp, 7, out)),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, vp(tabs.data_ptr()), 2, 64, ptp, 64, out)),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, vp(tabs.data_ptr()), 2, 64, ptp, 1 << 31, out)),
            (INVALID, L.lf_mle_fix_variables, (ctx.h, hp, 2, 1, ptp, 1, hp)),
            usable,
            # 5. overlap of an input range with out, a host pointer where device memory is due
            (INVALID, L.lf_spmv_t_device, (ctx.h, 0, out, vp(big.data_ptr() + 8 * RE))),
            (INVALID, L.lf_mle_fix_variables_device, (ctx.h, out, 2, 64, ptp, 1, vp(big.data_ptr() + 64 * RE * 8))),
            (INVALID, L.lf_witness_get_z_device, (ctx.h, wit.h, xp, C.cast(hp, vp))), (INVALID, L.lf_witness_mz_device, (ctx.h, wit.h, xp, C.cast(hp, vp))),
            (INVALID, L.lf_witness_get_fhat_device, (ctx.h, hs(wit), 1, C.cast(hp, vp))),
            usable,
        ]
        for k, chk in enumerate(checks):
            if chk is usable:
                usable()
                continue
            code, fn, args = chk
            assert _rc(fn, *args) == code, (k, fn.__name__)
        # a word >= p: in x, in a point, in a host array (on the host); in a device array (found by the kernel that reads it)
        bad = x.copy()
        bad[0, 1] = np.uint64(wl.P)
        assert _rc(L.lf_witness_get_z_device, ctx.h, wit.h, bad.ctypes.data_as(u64p), out) == INVALID
        badv = rand_ring(1, m, wl)
        badv[m - 1, RE - 1] = np.uint64(wl.P)
        assert _rc(L.lf_spmv_t, ctx.h, 0, badv.ctypes.data_as(u64p), hp) == INVALID
        assert _rc(L.lf_spmv_t_device, ctx.h, 0, vp(dev(badv).data_ptr()), out) == INVALID
        badt = rand_ring(3, 2 * 64, wl)
        badt[5, 0] = np.uint64(2**64 - 1)
        assert _rc(L.lf_mle_fix_variables_device, ctx.h, vp(dev(badt).data_ptr()), 2, 64, ptp, 3, out) == INVALID
        usable()
        # 1. a handle with another N: the context now holds a system of N = 320
        g5 = make_workload("G5", 0)
        other.load_ccs(g5)
        big2 = filled((g5.tau * g5.m, RE))
        assert _rc(L.lf_witness_get_fhat_device, other.h, hs(foreign), 1, vp(big2.data_ptr())) == INVALID
        assert _rc(L.lf_witness_mz_device, other.h, foreign.h, xp, vp(big2.data_ptr())) == INVALID
        # 4. a sharded context: the sharding model
        model.set_sharding_model(0, 2)
        model.load_ccs(wl)
        wm = api.Witness.from_w_ccs(model, wl.w_ccs)
        for fn, args in ((L.lf_witness_get_fhat_device, (model.h, hs(wm), 1, out)), (L.lf_witness_get_z_device, (model.h, wm.h, xp, out)),
                         (L.lf_witness_mz_device, (model.h, wm.h, xp, out)), (L.lf_spmv_t_device, (model.h, 0, vp(v.data_ptr()), out)),
                         (L.lf_mle_fix_variables_device, (model.h, vp(tabs.data_ptr()), 2, 64, ptp, 1, out))):
            assert _rc(fn, *args) == UNSUPPORTED, fn.__name__
        torch.cuda.synchronize()
        assert (big == PATTERN).all() and (big2 == PATTERN).all() and not hout.any()      # nothing was written by any refused call
        # fix_variables on the bare context, and the refused context still folds like the oracle
        one = api.mle_fix_variables(bare, rand_ring(3, 2 * 64, wl).reshape(2, 64, RE), pt[:1])
        assert (one == fix_np(rand_ring(3, 2 * 64, wl).reshape(2, 64, RE), embed(pt[0]), wl.ring)).all()
        _step_equals_oracle(ctx, wl)
    finally:
        for c in (ctx, other, bare, model):
            c.close()


@pytest.mark.parametrize("name", ["T8", "B6"])
def test_a_fold_step_next_to_the_tables_is_unchanged(name):
    wl = make_workload(name, 0)
    busy, sibling = Case(wl, ajtai=False), api.Context(0, ring=wl.ring)
    try:
        sibling.load_ccs(wl)
        parts = busy.wit.decompose(busy.ctx)
        api.get_fhat(busy.ctx, parts, device=True)
        busy.wit.mz(wl.x_ccs, device=True)
        zd = busy.wit.get_z(wl.x_ccs, device=True)
        v = dev(rand_ring(5, wl.m, wl))
        for j in range(wl.t):
            busy.ctx.mat_vec_mul_t(j, v)
        api.mle_fix_variables(busy.ctx, v.reshape(1, wl.m, wl.RE), rand_ring(6, 3, wl)[:, :wl.tau].copy())
        assert (host(zd) == wl.z()).all()
        _step_equals_oracle(sibling, wl)
        _step_equals_oracle(busy.ctx, wl)                    # ... and the context that built the tables folds like the oracle too
    finally:
        busy.close()
        sibling.close()
