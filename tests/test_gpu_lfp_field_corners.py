"""Frog-ring device arithmetic at the corners of its Montgomery words, word for word against Python integers.

Every LatticeFold+ kernel is built on mont_mul, add_p, sub_p and the lazy 160-bit sums of latticefold_amd/csrc/lfp_field.cuh.  Random operands and canonical
corners (0, 1, p - 1, (p +- 1) / 2) reach three of the classes (cy, o1, o2, v >= p) of mont_mul and leave the carry chains of the sums to chance: cy = 0 needs
a b = 0 (mod 2^64), o2 = 1 needs a b + m p = 2^128 exactly.  Every case here goes through an existing entry point of latticefold_amd/plus.py with operands from
tests/lfp_field_corners.py -- the grid of DEVICE words (placed through canon_of_word, so a to_mont on the way in produces exactly the word), the constructed
pairs, monomial rows that put one chosen product with a chosen sign into a lazy sum -- and is compared with that module's reference on Python integers (`%`),
which knows nothing of Montgomery form.  tests/test_lfp_field_corners_cpu.py pins the reference against the oracle on the same tables and proves, case by case,
that the operands reach the branches.  The transcript-driven entry points (the CCS linearization, the range check) and the decomposition are compared with
tests/lfplus_ccs_ref.py and the oracle."""
import numpy as np
import pytest
import torch

import lfp
import lfp_field_corners as fc
import lfplus_ccs_ref as cref
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
P, D = fc.P, fc.D


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, reference {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: device {int(got[tuple(bad[0])]):#x}, reference {int(want[tuple(bad[0])]):#x}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _loaded(n, seed=0xF1):
    """(context with a commitment matrix for n columns, the matrix)"""
    A = ref.rand_ring(seed, (1, n, D))
    c = plus.PlusContext(0)
    try:
        c.set_matrix(A)
    except Exception:
        c.close()
        raise
    return c, A


# ---- mont_mul directly: tensor_product, tensor ---------------------------------------------------------------------------------------------------------------
def test_tensor_product_on_the_grid_and_the_constructed_pairs():
    """mul_p(a, b) = mont_mul(mont_mul(a, b), R2): grid x grid, and every constructed pair on the diagonal of firsts x seconds"""
    ctx = plus.PlusContext(0)
    try:
        _same(ctx.tensor_product(fc.GRID, fc.GRID), fc.tensor_product(fc.GRID, fc.GRID), "tensor_product/grid")
        got = ctx.tensor_product(fc.PAIR_A, fc.PAIR_B)
        want = fc.tensor_product(fc.PAIR_A, fc.PAIR_B)
        k = len(fc.PAIRS)
        for i, name in enumerate(fc.PAIRS):
            assert int(got[i * k + i]) == int(want[i * k + i]), f"pair {name} {fc.PAIRS[name]}: device {int(got[i * k + i]):#x}, reference {int(want[i * k + i]):#x}"
        _same(got, want, "tensor_product/pairs")
        assert int(want[list(fc.PAIRS).index("o2 issue") * (k + 1)]) == fc.R2      # a b + m p = 2^128: mont_mul gives 2^64 - p, the product is 2^128 mod p
    finally:
        ctx.close()


def test_tensor_on_grid_points():
    ctx = plus.PlusContext(0)
    try:
        for name, r in fc.TENSOR_POINTS.items():
            _same(ctx.tensor(r), fc.tensor(r), "tensor/" + name)
    finally:
        ctx.close()


# ---- the signed lazy sums: ring_mul ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.ring_mul_cases()))
def test_ring_mul(name):
    """host arrays and device arrays; a broadcast case also as mode 0 with b replicated; one term also in place (out is a)"""
    a, b, broadcast = fc.ring_mul_cases()[name]
    want = fc.ring_mul_sum(a, b, broadcast)
    ctx = plus.PlusContext(0)
    try:
        _same(ctx.ring_mul(a, b, broadcast=broadcast), want, f"ring_mul/{name} (host)")
        got = ctx.ring_mul(_dev(a), b if broadcast else _dev(b), broadcast=broadcast)
        _same(_host(got), want, f"ring_mul/{name} (device)")
        if broadcast:
            rep = np.ascontiguousarray(np.broadcast_to(b[:, None, :], a.shape))
            _same(ctx.ring_mul(a, rep), want, f"ring_mul/{name} (replicated)")
        if a.shape[0] == 1:
            x = a[0].copy()
            assert ctx.ring_mul(x, b if broadcast else b[0], broadcast=broadcast, out=x) is x
            _same(x, want, f"ring_mul/{name} (in place, host)")
            xd = _dev(a[0])
            assert ctx.ring_mul(xd, b if broadcast else _dev(b[0]), broadcast=broadcast, out=xd) is xd
            _same(_host(xd), want, f"ring_mul/{name} (in place, device)")
    finally:
        ctx.close()


# ---- mont_mul + add_p chains: spmv -----------------------------------------------------------------------------------------------------------------------------
def test_spmv():
    """ring coefficients (k_spmv_ring), constant coefficients whose device words are grid words (k_spmv_ring_const), and the matrix of ones whose rows run
    add_p through sum = p - 1, p, 2^64 - 1 and 2^64"""
    mats, x = fc.spmv_case()
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrices(mats, n=x.shape[0])
        xd = _dev(x)
        for j, m in enumerate(mats):
            want = fc.spmv(m, x)
            _same(ctx.spmv(j, x), want, f"spmv/{j} (host)")
            _same(_host(ctx.spmv(j, xd)), want, f"spmv/{j} (device)")
    finally:
        ctx.close()


# ---- the generic sumcheck ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvars", fc.MLS_NVARS)
def test_mlsumcheck_round_messages_and_final_values(nvars):
    """every round message and the final values at challenges given from the grid (0, 1, p - 1, the value whose Montgomery word is 2^32, the to_mont corner
    operands) against prove_round / fix of the reference; nvars 1: one pair, 4: a partial group, 5: a full 16-pair group"""
    tables, terms, degree, ch = fc.mls_case(nvars)
    rt = ref.terms_as_rings(terms)
    T = tables.astype(object)
    ctx = plus.PlusContext(0)
    try:
        sc = plus.MLSumcheck(ctx, tables, plus.VPoly(terms, degree))
        for rnd in range(nvars):
            if rnd:
                T = ref.fix(T, ch[rnd - 1])
            msg = sc.prove_round(None if rnd == 0 else ch[rnd - 1])
            _same(msg, ref._u64(ref.prove_round(T, rt, degree)), f"mlsumcheck/nvars{nvars} round {rnd + 1}")
        fin = sc.final(ch[nvars - 1])
        want = ref._u64(ref.fix(T, ch[nvars - 1])[:, 0])
        _same(fin, want, f"mlsumcheck/nvars{nvars} final")
        _same(ref.g_at(fin, rt), ref._u64(ref.comb(want.astype(object), rt)), f"mlsumcheck/nvars{nvars} g(final)")
        sc.end()
    finally:
        ctx.close()


# ---- the CCS linearization ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvars", [4, 5])
@pytest.mark.parametrize("name", sorted(fc.SHAPES))
def test_ccs_linearize_and_verify(name, nvars):
    """a satisfied instance with a witness from the grid, matrices of placed grid words and (deg3) a constant coefficient whose Montgomery word is 2^32; the
    challenges are the transcript's, so the reference is tests/lfplus_ccs_ref.py on the oracle's transcript"""
    sh = fc.SHAPES[name]
    mats, f = fc.lin_case(name, nvars)
    seed = ref.rand_ring(0x5EED, (2, D))
    tr_o = lfp.Transcript()
    tr_o.absorb(seed)
    want = cref.linearize(tr_o, sh, f, mats)
    ctx, _ = _loaded(1 << nvars)
    try:
        tr = plus.PoseidonTranscript()
        tr.absorb(seed)
        shape = plus.CCSShape(*sh)
        linb, proof = plus.ComCCS(shape, tuple(mats), f, None).linearize(ctx, tr)
        for key in ("msgs", "r", "evals"):
            _same(proof[key], want[key], f"ccs_linearize/{name}/nvars{nvars} {key}")
        assert tr.get_challenge() == tr_o.challenge()
        tv = plus.PoseidonTranscript()
        tv.absorb(seed)
        ok, stage, ro = plus.ccs_verify(tv, shape, proof)
        assert ok and stage == 0, (ok, stage)
        _same(ro, want["r"], f"ccs_verify/{name}/nvars{nvars} point")
    finally:
        ctx.close()


# ---- the relation checks -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.SHAPES))
def test_relation_checks_accept_planted_products_and_reject_one_changed_word(name):
    """n = 64: the rows gather grid and monomial elements (ring coefficients: signed sums; constant coefficients: ONE unsigned sum per row), the reference's
    product row is planted as g_C; rows 0..11 carry the constructed pairs' products.  Accepted with first_bad == n; with one word of one product row changed
    by +-1, rejected at exactly that row.  The R1CS shape goes through r1cs_check and ccs_check, the degree-3 shape through ccs_check"""
    mats, f, rows = fc.check_case(name)
    n = f.shape[0]
    shape = plus.CCSShape(*fc.SHAPES[name])
    ctx, A = _loaded(n)
    try:
        cm = lfp.commit(A, f)
        amax = max(abs(fc.centre(w)) for w in f.reshape(-1))
        ctx.set_matrices(mats)

        def run(cm_f):
            out = [("ccs_check", ctx.ccs_check(cm_f, shape))]
            if name == "r1cs":
                out.append(("r1cs_check", ctx.r1cs_check(cm_f)))
            return out
        ctx.set_witness(f)
        for who, res in run(cm):
            assert res == (True, 0, n, amax), f"{who}/{name}: a satisfied instance gives {res}"
        for row, word, delta in fc.CHECK_BAD:
            g = f.copy()
            g[32 + row, word] = np.uint64((int(g[32 + row, word]) + delta) % P)
            ctx.set_witness(g)
            for who, (ok, failed, first_bad, _) in run(None):
                assert not ok and failed == plus.REL_R1CS and first_bad == row, f"{who}/{name}: word {word} of row {row} changed by {delta}: {(ok, failed, first_bad)}"
    finally:
        ctx.close()


def test_linb_check_on_grid_words():
    """nvars = 10: every witness word from the grid, both points constants whose Montgomery words are grid words, one constant-coefficient matrix of placed grid
    words: accepted with the reference's evaluations, rejected with any one evaluation word off by one"""
    f, r, mats, v = fc.linb_case()
    ctx, A = _loaded(f.shape[0])
    try:
        ctx.set_witness(f)
        cm = lfp.commit(A, f)
        amax = max(abs(fc.centre(w)) for w in f.reshape(-1))
        assert ctx.linb_check(cm, r, v, mats) == (True, 0, amax)
        for q in range(2):
            for pt in range(2):
                for word in range(D):
                    bad = v.copy()
                    bad[q, pt, word] = np.uint64((int(bad[q, pt, word]) + (1 if word % 2 else P - 1)) % P)
                    assert ctx.linb_check(cm, r, bad, mats) == (False, plus.REL_V, amax), (q, pt, word)
    finally:
        ctx.close()


# ---- the balanced digits -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", fc.DECOMP_BASES)
def test_decompose_at_the_digit_boundaries(B):
    """B odd, a power of two, even and no power of two (exact ties +-B/2), ceil(sqrt q) + 1; f holds (p +- 1) / 2, +-floor(B / 2), +-(floor(B / 2) + 1),
    +-(B floor(B / 2) + floor(B / 2)) and their neighbours among centred-small values.  Against the oracle, and the identities on Python integers"""
    f, _ = fc.decompose_f(B)
    n = f.shape[0]
    nv = n.bit_length() - 1
    r = np.zeros((nv, 2, D), dtype=np.uint64)
    r[:, :, 0] = fc.rows_u64([[fc.placed(fc.GRID[(2 * j + pt) % fc.NG]) for pt in range(2)] for j in range(nv)])
    ctx, A = _loaded(n, seed=0xDC + B % 97)
    try:
        got = ctx.decompose(f, None, B, r)
        want = lfp.decompose(f, A, B, r[:, 0], r[:, 1])
        for k in ("F0", "F1", "C0", "C1", "v0", "v1"):
            _same(got[k], want[k], f"decompose/B{B} {k}")
        F0, F1 = fc.decompose2(f, B)
        _same(got["F0"], F0, f"decompose/B{B} F0 (Python integers)")
        _same(got["F1"], F1, f"decompose/B{B} F1 (Python integers)")
        assert fc.decompose_identities(f, got["F0"], got["F1"], B)[0]
    finally:
        ctx.close()


# ---- one protocol-level case --------------------------------------------------------------------------------------------------------------------------------------
def test_range_check_with_ring_weights_on_grid_words(monkeypatch):
    """the smallest range check of test_range_check_matches_oracle (L = 1, one matrix, nvars = 14) with LFPLUS_RING_WEIGHTS=1 and an identity-like matrix whose
    diagonal cycles through placed grid words: k_wring<true>, k_wdot and the transposed products on grid words, against the oracle"""
    monkeypatch.setenv("LFPLUS_RING_WEIGHTS", "1")
    nvars, k = 14, 2
    n = 1 << nvars
    dp = plus.DecompParameters.for_frog(k)
    A = lfp.splitmix(1, 0, n * D).reshape(1, n, D)
    v = (lfp.splitmix(20, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    f = np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)
    mats = [fc.range_check_matrix(n)]
    ctx = plus.PlusContext(0)
    try:
        rg = plus.RgInstance.from_f(ctx, f, A, dp)
        inst = {"Mf": lfp.exp_dense(rg.D_f), "tau": rg.tau, "mtau": lfp.exp_dense(rg.m_tau_exp), "f": f}
        to, tp = lfp.Transcript(), plus.PoseidonTranscript()
        want = lfp.range_check(to, nvars, [inst], k, mats)
        got = plus.range_check([ctx], tp, mats)
        for key in ("msgs", "r", "e", "b", "v", "a", "bb", "c"):
            _same(got[key], want[key], f"range_check {key}")
        assert tp.get_challenge() == to.challenge()
        ok, stage, _ = plus.range_check_verify(plus.PoseidonTranscript(), got)
        assert ok and stage == 0
    finally:
        ctx.close()
