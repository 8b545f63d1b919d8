"""Shapes, inputs and the reference linearization of the committed-CCS tests (tests/test_lfplus_ccs_cpu.py, tests/test_gpu_lfplus_ccs.py): Python, none of it
the code under test.  The prover is tests/lfplus_mlsumcheck_ref.py's literal MLSumcheck (pinned to the oracle's lfp.r1cs_linearize by
test_lfplus_mlsumcheck_cpu.py) on the tables [eq(r, .), g_0, .., g_{t-1}] with the terms c_i * eq * prod_{j in S_i} g_j at degree d + 1; mle(f)(ro) is a sum
of Python integers; Fiat-Shamir is the oracle's transcript (lfp.Transcript).

A shape is (t, multisets, coeffs): coeffs are Python integers (constant polynomials) or (16,) ring elements."""
import numpy as np

import lfp
import lfplus_mlsumcheck_ref as ref

P, D = lfp.P, lfp.D
R1CS = (3, [[0, 1], [2]], [1, -1])


def _g(seed):
    return ref.rand_ring(0xCC5 + seed, (D,))


def shape(name):
    if name == "r1cs":
        return R1CS
    if name == "a":      # the longest chain, a repeated index, degree 8
        return 1, [[0] * 7, [0]], [1, -1]
    if name == "b":      # a Plonk-style gate q_M a b + q_L a + q_R b + q_O c + q_C: wires M_0..M_2, selectors M_3..M_7; coefficients 1, -1, the constant 5, general, 0
        return 8, [[3, 0, 1], [4, 0], [5, 1], [6, 2], [7]], [1, -1, 5, _g(1), 0]
    if name == "b4":     # the same gate over four matrices (the fold test)
        return 4, [[3, 0, 1], [0], [3, 1], [3, 2], [3]], [1, -1, 5, _g(2), 0]
    if name == "c":      # eight single-factor terms: d = 1, no product at all
        return 4, [[0], [1], [2], [3], [0], [1], [2], [3]], [1, -1, 7, 0, P - 2, 1, -1, 3]
    if name == "c-gen":  # the same with two general coefficients: the only products are theirs
        return 4, [[0], [1], [2], [3], [0], [1], [2], [3]], [1, -1, 7, _g(3), 0, 1, _g(4), -1]
    if name == "d":      # S_off[q] = 16 exactly: eight products in flight at one level, general coefficients on top
        return 8, [[0, 1], [2, 3], [4, 5], [6, 7], [0, 2], [1, 3], [4, 6], [5, 7]], [_g(5), _g(6), 1, -1, _g(7), 3, _g(8), 1]
    if name == "e":      # t = 8, d = 7, all eight matrices in use, a general coefficient behind the longest chain
        return 8, [[0, 1, 2, 3, 4, 5, 6], [7, 0]], [_g(9), -1]
    if name == "cube":   # x^3 - x (the relation check)
        return 1, [[0, 0, 0], [0]], [1, -1]
    raise KeyError(name)


def coef_ring(c):
    return ref._u64(ref.const(c)) if isinstance(c, (int, np.integer)) else np.asarray(c, dtype=np.uint64)


def terms_of(sh):
    """the product list over the tables [eq, g_0, ..]: eq is table 0 and a factor of every term"""
    t, S, c = sh
    return [(coef_ring(ci), [0] + [1 + j for j in Si]) for Si, ci in zip(S, c)]


def degree_of(sh):
    return max(len(Si) for Si in sh[1])


def matrices(t, n, seed, const_from=None, per_row=1):
    """t random n x n CSR matrices with ring coefficients; matrices const_from.. have constant coefficients (the one-word path of the SpMV)"""
    out = []
    for j in range(t):
        rp, col, val = ref.rand_csr(seed * 17 + j, n, per_row)
        if const_from is not None and j >= const_from:
            val = val.copy()
            val[:, 1:] = 0
        out.append((rp, col, val))
    return out


def ragged_matrix(n, seed):
    """ring-valued, 0-3 entries per row: empty rows and multi-entry rows"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 4, size=n)
    cnt[0], cnt[n - 1] = 0, 3
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    return rp, rng.integers(0, n, size=int(rp[-1])).astype(np.uint32), ref.rand_ring(seed * 7 + 1, (int(rp[-1]), D))


def satisfied_r1cs(n, seed):
    """(f, (A, B, C)) with (A f) o (B f) = C f row by row: f holds the ring constants 0 / 1, A and B select random entries, C selects the factor that decides the
    product (the first when the second is 1, else the second)"""
    rng = np.random.default_rng(seed)
    f = np.zeros((n, D), dtype=np.uint64)
    f[:, 0] = rng.integers(0, 2, size=n).astype(np.uint64)
    f[0, 0], f[n - 1, 0] = 1, 0
    a, b = rng.integers(0, n, size=n), rng.integers(0, n, size=n)
    c = np.where(f[b, 0] == 1, a, b)
    one = np.zeros((n, D), dtype=np.uint64)
    one[:, 0] = 1
    rp = np.arange(n + 1, dtype=np.uint32)
    return f, tuple((rp, x.astype(np.uint32), one) for x in (a, b, c))


def mle_at(f, point):
    """mle(f)(point) with Python integers"""
    w = ref.eq_table(point)[:, 0].astype(object)
    return ref._u64((ref._obj(f) * w[:, None]).sum(axis=0) % P)


def seed_transcripts(mine, oracle, seed=0x5EED):
    x = ref.rand_ring(seed, (2, D))
    mine.absorb(x)
    oracle.absorb(x)


def linearize(tr, sh, f, mats):
    """the protocol of lfplus_ccs_linearize on the oracle transcript `tr` -> dict(msgs, r, evals, nvars)"""
    f = np.asarray(f, dtype=np.uint64)
    nvars = f.shape[0].bit_length() - 1
    r = [tr.challenge() for _ in range(nvars)]
    tables = np.stack([ref.eq_table(r)] + [ref.spmv(m, f) for m in mats])
    msgs, point, final = ref.prove(tr, tables, terms_of(sh), degree_of(sh) + 1)
    evals = np.concatenate([mle_at(f, point)[None], final[1:]])
    tr.absorb(evals)
    return {"msgs": msgs, "r": point, "evals": evals, "nvars": nvars}


def replay(tr, sh, proof):
    """the verifier's transcript schedule alone (no check): what the oracle side of a fold needs to stand where the prover stands"""
    nvars, d = proof["nvars"], degree_of(sh)
    for _ in range(nvars):
        tr.challenge()
    ref.prologue(tr, nvars, d + 1)
    for i in range(nvars):
        ref.transcript_round(tr, proof["msgs"][i])
    tr.absorb(np.ascontiguousarray(proof["evals"], dtype=np.uint64))


_CASES = {}


def case(name, nvars, fill=None):
    """(shape, f, mats, proof, next challenge) of a named case on a seeded oracle transcript: computed once, shared, never written.  fill: every word of f and of
    the matrix values is this number (the saturation cases)"""
    key = (name, nvars, fill)
    if key not in _CASES:
        sh = shape(name)
        n = 1 << nvars
        f = ref.rand_ring(0xF0 + nvars + 13 * len(name), (n, D))
        mats = matrices(sh[0], n, 0x40 + nvars, const_from=3 if name in ("b", "b4") else None)
        if fill is not None:
            f = np.full((n, D), fill, dtype=np.uint64)
            mats = [(rp, col, np.full(val.shape, fill, dtype=np.uint64)) for rp, col, val in mats]
        tr = lfp.Transcript()
        tr.absorb(ref.rand_ring(0x5EED, (2, D)))
        proof = linearize(tr, sh, f, mats)
        for a in (f, proof["msgs"], proof["r"], proof["evals"]):
            a.setflags(write=False)
        _CASES[key] = (sh, f, mats, proof, tr.challenge())
    return _CASES[key]
