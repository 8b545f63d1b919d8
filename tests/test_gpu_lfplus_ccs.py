"""Committed CCS instances on the GPU (lfplus_ccs_linearize, lfplus_ccs_check; include/lfplus.h), word for word against yardsticks that are not the code under
test: the oracle's lfp.r1cs_linearize at the R1CS shape (the anchor: the one place the reference pins the protocol), the literal Python prover of
tests/lfplus_mlsumcheck_ref.py on [eq, g_0 ..] for every other shape (tests/lfplus_ccs_ref.py), and the oracle's cm_prove / decompose / verifiers for the fold
that follows a linearization.  Self-consistent, pinned to the reference at the R1CS shape."""
import ctypes as C

import numpy as np
import pytest

import lfp
import lfplus_ccs_ref as cref
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
P, D = plus.P, plus.D
u64p = plus.u64p
E_ARG = plus.E_ARG


def L():
    return plus._lib()


def err(c):
    return L().lfplus_last_error(c.h).decode()


def _ctx(n, kappa=1, seed=0xA0):
    c = plus.PlusContext(0)
    c.set_matrix(ref.rand_ring(seed + kappa, (kappa, n, D)))
    return c


def _seeded():
    t = plus.PoseidonTranscript()
    t.absorb(ref.rand_ring(0x5EED, (2, D)))
    return t


def _linearize(c, tr, sh, f, mats, resident=False):
    inst = plus.ComCCS(plus.CCSShape(*sh), tuple(mats), f, None)
    return inst.linearize(c, tr, resident=resident)


def _same(proof, want):
    for key in ("msgs", "r", "evals"):
        assert np.array_equal(proof[key], want[key]), key


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------------------------------------
def _anchor(nvars, r1cs, f):
    n = 1 << nvars
    tr_o = lfp.Transcript()
    tr_o.absorb(ref.rand_ring(0x5EED, (2, D)))
    want = lfp.r1cs_linearize(tr_o, nvars, f, r1cs)
    c, c2 = _ctx(n), _ctx(n)
    try:
        tr = _seeded()
        linb, proof = _linearize(c, tr, cref.R1CS, f, r1cs)
        assert proof["msgs"].shape == (nvars, 4, D) and proof["evals"].shape == (4, D)
        assert np.array_equal(proof["msgs"], want["msgs"]) and np.array_equal(proof["r"], want["r"])
        assert np.array_equal(proof["evals"][1:], want["evals"][1:]) and np.array_equal(proof["evals"][0], want["evals"][0])
        assert np.array_equal(proof["evals"][0], cref.mle_at(f, want["r"]))
        assert tr.get_challenge() == tr_o.challenge()
        tr2 = _seeded()
        linb2, proof2 = plus.ComR1CS(tuple(r1cs), None, f, None).linearize(c2, tr2)
        _same(proof, proof2)
        assert linb["r"] is proof["r"] and linb["v"] is proof["evals"]
    finally:
        c.close()
        c2.close()


@pytest.mark.parametrize("nvars", [1, 4, 5, 6, 10])
def test_anchor_r1cs_shape_equals_the_oracle_and_the_hard_wired_path(nvars):
    """nvars 1: one pair, no fused round; 4 and 5: 8 and 16 pairs, a partial and an exactly full 16-pair group; 6: two groups; 10: every later round fused, down
    to one pair"""
    n = 1 << nvars
    _anchor(nvars, [ref.rand_csr(0x90 + 3 * nvars + q, n, 1) for q in range(3)], ref.rand_ring(0x91 + nvars, (n, D)))


def test_anchor_ring_valued_ragged_rows():
    n = 32
    _anchor(5, [cref.ragged_matrix(n, 0x31 + q) for q in range(3)], ref.rand_ring(0x97, (n, D)))


# ---- 2. general shapes, 3. saturation ---------------------------------------------------------------------------------------------------------------------------
def _check_case(name, nvars, fill=None, c=None):
    sh, f, mats, want, nxt = cref.case(name, nvars, fill)
    own = c is None
    c = _ctx(1 << nvars) if own else c
    try:
        tr = _seeded()
        linb, proof = _linearize(c, tr, sh, f, mats)
        d = cref.degree_of(sh)
        assert proof["msgs"].shape == (nvars, d + 2, D) and proof["evals"].shape == (1 + sh[0], D)
        _same(proof, want)
        assert tr.get_challenge() == nxt
        return proof
    finally:
        if own:
            c.close()


@pytest.mark.parametrize("nvars", [1, 2, 5, 6])
@pytest.mark.parametrize("name", ["a", "b", "c", "c-gen", "d", "e"])
def test_general_shapes_equal_the_python_reference(name, nvars):
    """(a) the longest chain, a repeated index, degree 8; (b) a Plonk-style gate, t = 8, coefficients 1, -1, 5, general, 0; (c) eight single-factor terms, no
    product (c-gen: the only products are two general coefficients'); (d) S_off[q] = 16, eight chains in flight, the LDS carve at its maximum; (e) t = 8, d = 7"""
    _check_case(name, nvars)


@pytest.mark.parametrize("fill", [P - 1, (P - 1) // 2])
@pytest.mark.parametrize("name", ["a", "r1cs"])
def test_saturated_operands(name, fill):
    """every word of f and of the matrix values p - 1, and (p - 1) / 2: the lazy 160-bit sums and the chain reductions at their bounds"""
    _check_case(name, 4, fill)


# ---- 4. grid-stride loop and switches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"LFPLUS_CCS_BLOCKS": "1"}, {"LFPLUS_CCS_BLOCKS": "3"}, {"LFPLUS_CM_UNFUSED": "1"}, {"LFPLUS_CM_UNFUSED": "1", "LFPLUS_CCS_BLOCKS": "3"}])
def test_block_cap_and_unfused_fix_give_the_default_words(env, monkeypatch):
    c = _ctx(1 << 7)
    try:
        default = _check_case("b", 7, c=c)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = _check_case("b", 7, c=c)
        _same(got, default)
    finally:
        c.close()


# ---- 5. the relation check --------------------------------------------------------------------------------------------------------------------------------------
def _cube_instance(n, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros((n, D), dtype=np.uint64)
    f[:, 0] = np.array([0, 1, P - 1], dtype=np.uint64)[rng.integers(0, 3, size=n)]
    f[1, 0] = P - 1
    return f, [lfp.identity_csr(n)]


@pytest.mark.parametrize("nvars", [5, 10])
@pytest.mark.parametrize("name", ["cube", "r1cs"])
def test_relation_check(name, nvars):
    n, kappa = 1 << nvars, 2
    sh = plus.CCSShape(*cref.shape(name))
    f, mats = _cube_instance(n, 0x51 + nvars) if name == "cube" else cref.satisfied_r1cs(n, 0x52 + nvars)
    c = _ctx(n, kappa)
    try:
        inst = plus.ComCCS.new(c, sh, mats, f)
        assert np.array_equal(inst.cm_f, lfp.commit(ref.rand_ring(0xA0 + kappa, (kappa, n, D)), f))
        assert inst.check_relation(c) == (True, 0, n, 1)
        if name == "r1cs":
            assert c.r1cs_check(inst.cm_f, mats) == (True, 0, n, 1)
        # the norm rule is absmax < bound
        assert inst.check_relation(c, bound=1) == (False, plus.REL_NORM, n, 1) and inst.check_relation(c, bound=2) == (True, 0, n, 1)
        # a wrong commitment
        cm = inst.cm_f.copy()
        cm[kappa - 1, 7] ^= np.uint64(1)
        assert c.ccs_check(cm, sh, mats) == (False, plus.REL_CM, n, 1)
        assert c.ccs_check(None, sh, mats) == (True, 0, n, 1)
        # resident matrices
        c.set_matrices(mats)
        assert inst.check_relation(c, resident=True) == (True, 0, n, 1)
        # broken at row 0, a middle row and row n - 1 (2^3 != 2; 2 * 2 != 2): the residual alone fails, the commitment is the broken witness's
        for row in (0, n // 2 + 3, n - 1):
            g = f.copy()
            g[row] = 0
            g[row, 0] = 2
            if name == "r1cs":      # the row must read the changed entry: point all three matrices of that row at it
                m2 = [(rp, col.copy(), val) for rp, col, val in mats]
                for m in m2:
                    m[1][row] = row
            else:
                m2 = mats
            bad = plus.ComCCS.new(c, sh, m2, g)
            got = bad.check_relation(c)
            if name == "r1cs":
                # other rows that read entry `row` through their own matrices may fail too: the first failing row is what a Python pass over the rows finds
                ga, gb, gc = (ref.spmv(m, g).astype(object) for m in m2)
                res = (ref.rmul(ga, gb) - gc) % P
                first = int(np.flatnonzero(res.any(axis=1))[0])
                assert first <= row
            else:
                first = row
            assert got == (False, plus.REL_CCS, first, 2), (row, got)
            # both components at once, and the norm on top
            assert c.ccs_check(inst.cm_f, sh, m2, bound=2) == (False, plus.REL_CM | plus.REL_CCS | plus.REL_NORM, first, 2)
        # the context is as usable as before: the good instance again
        assert inst.check_relation(c) == (True, 0, n, 1)
    finally:
        c.close()


# ---- 6. the fold goes through -----------------------------------------------------------------------------------------------------------------------------------
def _small_witness(n, seed):
    v = (lfp.splitmix(seed, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    return np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)


def test_linearize_then_mlin_then_decompose_equals_the_oracle():
    """One instance of the gate over four matrices at nvars 14 (the smallest n of the cm_prove tests: kappa k d l d < n): linearized on the device, folded by the
    existing mlin with nM = 4 and decomposed; the oracle side replays the linearization's transcript schedule and runs rg_from_f / cm_prove / decompose.  L = 1:
    the oracle's cm_prove with four matrices takes 1.9 s per instance on the CPU, and two instances would make this one case the slowest of the slice"""
    nvars, kappa, k, Lq = 14, 1, 2, 1
    B = plus.estimate_bound(16 * 128, Lq, D, k) + 1      # utils::estimate_bound (utils.rs:102-112), as the prover tests choose it: the folded witness fits two base-B digits
    n = 1 << nvars
    dp = plus.DecompParameters.for_frog(k)
    params = plus.LinParameters(kappa, dp)
    sh = cref.shape("b4")
    A = lfp.splitmix(3, 0, kappa * n * D).reshape(kappa, n, D) % np.uint64(P)
    mats = []
    for j in range(4):      # constant coefficients (the range relation needs them), small ones
        rp, col, val = ref.rand_csr(0x70 + j, n, 1)
        val = val.copy()
        val[:, 1:] = 0
        val[:, 0] %= np.uint64(5)
        mats.append((rp, col, val))
    fs = [_small_witness(n, 40 + l) for l in range(Lq)]
    ctxs, res = [], plus.RESIDENT(4)
    try:
        for l in range(max(Lq, 2)):      # (the second context receives F1)
            c = plus.PlusContext(0)
            if l == 0:
                c.set_matrix(A)
                c.set_matrices(mats)
            else:
                c.share_matrix(ctxs[0])
                c.share_matrices(ctxs[0])
            ctxs.append(c)
        tr, tr_o = _seeded(), lfp.Transcript()
        tr_o.absorb(ref.rand_ring(0x5EED, (2, D)))
        proofs = []
        for l in range(Lq):
            linb, proof = _linearize(ctxs[l], tr, sh, fs[l], mats, resident=True)
            proofs.append(proof)
            cref.replay(tr_o, sh, proof)
            # the LinB of the linearization holds on the device (both points are ro)
            r2 = np.zeros((nvars, 2, D), dtype=np.uint64)
            r2[:, 0, 0] = r2[:, 1, 0] = proof["r"]
            v2 = np.repeat(proof["evals"][:, None, :], 2, axis=1)
            assert ctxs[l].linb_check(None, r2, v2, res)[:2] == (True, 0)
        verifier_o = tr_o.clone()
        linb2x, cm = plus.mlin(ctxs[:Lq], tr, params, res)
        insts = []
        for f in fs:
            rg = lfp.rg_from_f(f, A, dp.b, dp.k, dp.l)
            tau_i = np.array([int(t) if int(t) <= P // 2 else int(t) - P for t in rg["tau"]], dtype=np.int8)
            insts.append({"Mf": lfp.exp_dense(rg["Df"]), "tau": rg["tau"], "mtau": lfp.exp_dense(tau_i), "f": f, "comMf": rg["comMf"],
                          "fcoms": np.stack([rg["cm_f"], rg["C_Mf"], rg["cm_mtau"]])})
        want = lfp.cm_prove(tr_o, nvars, insts, k, dp.l, kappa, mats)
        for key in ("msgs", "r", "e", "b", "v", "a", "bb", "c", "comh", "pa", "ea", "pb", "eb", "ro", "cm_g", "vo"):
            assert np.array_equal(cm[key], want[key]), key
        assert np.array_equal(cm["fcoms"], np.stack([i["fcoms"] for i in insts]))
        g, cm_g, vo = want["g"][0], want["cm_g"][0], want["vo"][0]
        for i in range(1, Lq):
            g, cm_g, vo = lfp.addmod(g, want["g"][i]), lfp.addmod(cm_g, want["cm_g"][i]), lfp.addmod(vo, want["vo"][i])
        assert np.array_equal(linb2x["cm_g"], cm_g) and np.array_equal(linb2x["vo"], vo)
        r_pairs = plus._ro_pairs(linb2x["ro"])
        dec = ctxs[0].decompose(None, None, B, r_pairs, res, into=(ctxs[0], ctxs[1]))
        wd = lfp.decompose(g, A, B, np.ascontiguousarray(r_pairs[:, 0]), np.ascontiguousarray(r_pairs[:, 1]), mats)
        for key in ("C0", "C1", "v0", "v1"):
            assert np.array_equal(dec[key], wd[key]), key
        assert np.array_equal(ctxs[0].get_witness(), wd["F0"]) and np.array_equal(ctxs[1].get_witness(), wd["F1"])
        assert tr.get_challenge() == tr_o.challenge()
        # the verifiers: each linearization (unsatisfied random instances are rejected in round 0 by design: only the transcript matters here), the oracle's
        # CmProof and DecompProof verifiers, and both accumulator halves as LinB instances on the device
        assert lfp.cm_verify(verifier_o, cm, [i["fcoms"] for i in insts])[0] == 0
        assert lfp.decomp_verify(dec, cm_g, vo, B) == 0
        for i in range(2):
            assert ctxs[i].linb_check(dec[f"C{i}"], r_pairs, dec[f"v{i}"], res)[:2] == (True, 0)
    finally:
        for c in ctxs:
            c.close()


# ---- 7. refusals on the device ----------------------------------------------------------------------------------------------------------------------------------
def _raw_linearize(c, tr, desc, mats, outs):
    keep, rp, cp, vp = plus._csr_args(mats)
    return L().lfplus_ccs_linearize(c.h, tr.h, C.byref(desc), rp, cp, vp, *[o.ctypes.data_as(u64p) for o in outs])


def test_refusals_leave_context_and_transcript_alone():
    nvars = 4
    n = 1 << nvars
    sh, f, mats, want, nxt = cref.case("b", nvars)
    shape = plus.CCSShape(*sh)
    d = shape.desc()
    SENT = np.uint64(0x5A5A5A5A)
    outs = [np.full((nvars, 5, D), SENT), np.full(nvars, SENT), np.full((9, D), SENT)]
    tr = _seeded()
    fresh = _seeded().get_challenge()
    c = _ctx(n)
    sharded, odd, bare = plus.PlusContext(0), plus.PlusContext(0), _ctx(n)
    try:
        # no witness
        assert _raw_linearize(bare, tr, d, mats, outs) == E_ARG and "resident witness" in err(bare)
        # a sharded context (the timing model stands in for a transport)
        sharded.set_sharding_model(0, 2)
        assert _raw_linearize(sharded, tr, d, mats, outs) == E_ARG and "sharded" in err(sharded)
        failed = C.c_uint()
        keep, rp, cp, vp = plus._csr_args(mats)
        assert L().lfplus_ccs_check(sharded.h, None, C.byref(d), rp, cp, vp, 0, C.byref(failed), None, None) == E_ARG and "sharded" in err(sharded)
        # n not a power of two
        odd.set_matrix(ref.rand_ring(0xA7, (1, 24, D)))
        odd.set_witness(ref.rand_ring(0xA8, (24, D)))
        m24 = cref.matrices(8, 24, 0x33)
        assert _raw_linearize(odd, tr, d, m24, outs) == E_ARG and "2^nvars" in err(odd)
        assert L().lfplus_ccs_check(odd.h, None, C.byref(d), *plus._csr_args(m24)[1:], 0, C.byref(failed), None, None) == E_ARG and "power of two" in err(odd)
        # on the loaded context: the shape's refusals come first, in the stated order, whatever else is wrong
        c.set_witness(f)
        c.set_matrices(mats[:3])
        assert _raw_linearize(c, tr, d, plus.RESIDENT(8), outs) == E_ARG and "do not number t" in err(c)
        assert L().lfplus_ccs_check(c.h, None, C.byref(d), None, None, None, 0, C.byref(failed), None, None) == E_ARG
        for bad, word in ((plus.CCSShape(9, sh[1], sh[2]), "envelope"), (plus.CCSShape(8, [[0] * 8], [1]), "more than 7"), (plus.CCSShape(8, [[0, 8]], [1]), ">= t"),
                          (plus.CCSShape(8, [[0] * 6, [1] * 6, [2] * 5], [1, 1, 1]), "more than 16"), (plus.CCSShape(8, [[0], []], [1, 1]), "strictly increasing")):
            assert _raw_linearize(c, tr, bad.desc(), plus.RESIDENT(8), outs) == E_ARG and word in err(c), word
        big = plus.CCSShape(*sh)
        big.coeffs[3, 9] = P
        assert _raw_linearize(c, tr, big.desc(), mats, outs) == E_ARG and "non-canonical coefficient" in err(c)
        # a malformed CSR array of the caller's
        rp0, col0, val0 = mats[5]
        worse = list(mats)
        worse[5] = (rp0, np.where(np.arange(col0.size) == 3, n, col0).astype(np.uint32), val0)
        assert _raw_linearize(c, tr, d, worse, outs) == E_ARG and "column index" in err(c)
        assert L().lfplus_ccs_linearize(c.h, None, C.byref(d), None, None, None, *[o.ctypes.data_as(u64p) for o in outs]) == E_ARG
        assert all((o == SENT).all() for o in outs), "a refused call writes nothing"
        assert tr.clone().get_challenge() == fresh, "a refused call leaves the transcript alone"
        assert np.array_equal(c.get_witness(), f)
        # a good call on the same context gives the reference words
        linb, proof = _linearize(c, tr, sh, f, mats)
        _same(proof, want)
        assert tr.get_challenge() == nxt
    finally:
        for x in (c, sharded, odd, bare):
            x.close()
