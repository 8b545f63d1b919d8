"""The reference prover and verifier of the LatticeFold+ generic sumcheck tests (tests/test_lfplus_mlsumcheck_cpu.py, tests/test_gpu_lfplus_mlsumcheck.py):
Python, none of it the code under test.  Ring arithmetic on Z_p[X]/(X^16 + 1) is Python integers in numpy object arrays (the schoolbook negacyclic product);
Fiat-Shamir is the oracle's transcript (lfp.Transcript).  The prover follows utils/sumcheck/prover.rs:111-143 literally -- per pair: the values at 0 and at 1,
the step, repeated addition of the step, the comb function at every point, the sum over the pairs -- and is NOT derived from the product's coefficients.  The
verifier restates verify_as_subprotocol (utils/sumcheck.rs:84-104, verifier.rs:92-257) with the coefficient-wise Lagrange form.  test_lfplus_mlsumcheck_cpu.py
pins this file to the oracle's lfp.r1cs_linearize.

A polynomial is a list of terms [(coef, [indices])], coef a ring element ((16,) words); tables are (T, n, 16); a challenge is one F_p word."""
import numpy as np

import lfp

P, D = lfp.P, lfp.D


def _obj(a):
    return np.asarray(a).astype(object)


def _u64(a):
    return np.asarray(a % P if a.dtype == object else a).astype(np.uint64)


def rmul(a, b):
    """negacyclic product of (..., 16) object arrays, reduced"""
    a, b = np.broadcast_arrays(_obj(a), _obj(b))
    out = np.zeros(a.shape, dtype=object)
    for j in range(D):
        for k in range(D):
            t = a[..., j] * b[..., k]
            if j + k < D:
                out[..., j + k] = out[..., j + k] + t
            else:
                out[..., j + k - D] = out[..., j + k - D] - t
    return out % P


def const(v):
    e = np.zeros(D, dtype=object)
    e[0] = int(v) % P
    return e


def comb(vals, terms):
    """the comb function on (T, ..., 16) values: sum_i coef_i * prod_{k in indices_i} vals[k]"""
    acc = 0
    for coef, idx in terms:
        pr = vals[idx[0]]
        for k in idx[1:]:
            pr = rmul(pr, vals[k])
        acc = (acc + rmul(pr, _obj(coef))) % P
    return acc


def prove_round(tables, terms, degree):
    """prover.rs:111-143 on the current tables (T, n, 16) -> (degree + 1, 16)"""
    v0, v1 = tables[:, 0::2], tables[:, 1::2]
    lev = [comb(v0, terms), comb(v1, terms)]
    steps, vals = (v1 - v0) % P, v1
    for _ in range(2, degree + 1):
        vals = (vals + steps) % P
        lev.append(comb(vals, terms))
    return np.stack([l.sum(axis=0) % P for l in lev[:degree + 1]])


def fix(tables, r):
    """DenseMultilinearExtension::fix_variables of the lowest variable: new[j] = old[2j] + r (old[2j+1] - old[2j]), coefficient by coefficient"""
    v0, v1 = tables[:, 0::2], tables[:, 1::2]
    return (v0 + int(r) * ((v1 - v0) % P)) % P


def prologue(tr, nvars, degree):
    tr.absorb(_u64(const(nvars)))
    tr.absorb(_u64(const(degree)))


def transcript_round(tr, evals):
    tr.absorb(_u64(evals))
    r = tr.challenge()
    tr.absorb(_u64(const(r)))
    return r


def prove(tr, tables, terms, degree):
    """prove_as_subprotocol on the oracle transcript `tr` -> (msgs (nvars, degree + 1, 16), point (nvars,), final (T, 16): the tables at the point)"""
    tables = _obj(tables)
    nvars = tables.shape[1].bit_length() - 1
    prologue(tr, nvars, degree)
    msgs, point = [], []
    for _ in range(nvars):
        if point:
            tables = fix(tables, point[-1])
        msgs.append(prove_round(tables, terms, degree))
        point.append(transcript_round(tr, msgs[-1]))
    return _u64(np.stack(msgs)), np.array(point, dtype=np.uint64), _u64(fix(tables, point[-1])[:, 0])


def hypercube_sum(tables, terms):
    """sum of g over {0,1}^nvars, brute force"""
    return _u64(comb(_obj(tables), terms).sum(axis=0) % P)


def interpolate(p_i, at):
    """sum_i p_i[i] prod_{j != i} (at - j) / (i - j), coefficient-wise (oracle lfp_protocol.c ring_sumcheck_verify; verifier.rs:139-257)"""
    n, res = len(p_i), np.zeros(D, dtype=object)
    for i in range(n):
        num, den = 1, 1
        for j in range(n):
            if j != i:
                num = num * (int(at) - j) % P
                den = den * (i - j) % P
        res = (res + _obj(p_i[i]) * (num * pow(den, P - 2, P) % P)) % P
    return res


def verify(tr, nvars, degree, claimed_sum, msgs):
    """verify_as_subprotocol -> (ok, point, expected or the failing round): the transcript runs over every round first, the checks follow"""
    msgs = np.asarray(msgs, dtype=np.uint64).reshape(nvars, degree + 1, D)
    prologue(tr, nvars, degree)
    point = np.array([transcript_round(tr, msgs[i]) for i in range(nvars)], dtype=np.uint64)
    expected = _obj(claimed_sum)
    for i in range(nvars):
        if not np.array_equal((_obj(msgs[i, 0]) + _obj(msgs[i, 1])) % P, expected):
            return False, point, i
        expected = interpolate(msgs[i], point[i])
    return True, point, _u64(expected)


def g_at(final, terms):
    """g evaluated on the tables' values at the point (T, 16)"""
    return _u64(comb(_obj(final), terms))


def extract_sum(msgs):
    m = _obj(msgs).reshape(-1, D)
    return _u64((m[0] + m[1]) % P)


# ---- the R1CS shape: the tables and terms whose sumcheck is ComR1CS::linearize's (r1cs.rs:76-139) ---------------------------------------------------------------
def rand_ring(seed, shape):
    return (lfp.splitmix(seed, 0, int(np.prod(shape))) % np.uint64(P)).reshape(shape)


def rand_csr(seed, n, per_row):
    """n x n CSR with ring coefficients, per_row entries in every row"""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, n, size=n * per_row).astype(np.uint32)
    return np.arange(0, n * per_row + 1, per_row, dtype=np.uint32), col, rand_ring(seed * 31 + 5, (n * per_row, D))


def spmv(mat, f):
    """M f with the oracle's ring product"""
    rowptr, col, val = mat
    out = np.zeros((rowptr.size - 1, D), dtype=object)
    for r in range(rowptr.size - 1):
        for k in range(rowptr[r], rowptr[r + 1]):
            out[r] = out[r] + _obj(lfp.ring_mul(val[k], f[col[k]]))
    return _u64(out % P)


def eq_table(r):
    """eq(r, x) for x in {0,1}^nvars as constant polynomials, bit i of x paired with r[i]"""
    w = [1]
    for ri in r:                      # (appending puts the newest variable in the highest bit)
        ri = int(ri)
        w = [x * (1 - ri) % P for x in w] + [x * ri % P for x in w]
    out = np.zeros((len(w), D), dtype=np.uint64)
    out[:, 0] = np.array(w, dtype=object).astype(np.uint64)
    return out


R1CS_TERMS = [(1, [0, 1, 2]), (P - 1, [0, 3])]


def r1cs_tables(r, f, r1cs):
    """(eq(r, .), M_A f, M_B f, M_C f): with R1CS_TERMS at degree 3 this is the polynomial ComR1CS::linearize runs its sumcheck on"""
    return np.stack([eq_table(r)] + [spmv(m, f) for m in r1cs])


def terms_as_rings(terms):
    return [(_u64(const(c)) if isinstance(c, (int, np.integer)) else np.asarray(c, dtype=np.uint64), ix) for c, ix in terms]


# ---- inputs: the shapes of tests/mlsumcheck_ref.py on the Frog ring ------------------------------------------------------------------------------------------------
def shape_a(nvars):
    """the reference's own rand_poly(nv, (2, 5), 3) (utils/sumcheck/utils.rs:186-230): three terms over DISJOINT tables, 2-4 factors and a random coefficient each"""
    rng = np.random.default_rng(11 + nvars)
    terms, T = [], 0
    for i in range(3):
        k = int(rng.integers(2, 5))
        terms.append((rand_ring(1000 + 7 * i + nvars, (D,)), list(range(T, T + k))))
        T += k
    return rand_ring(0xA1 + nvars, (T, 1 << nvars, D)), terms, max(len(ix) for _, ix in terms)


def shape_b(nvars):
    """sharing: two terms share table 1, a square, a cube, a single-factor term"""
    c = rand_ring(0xB0 + nvars, (5, D))
    return rand_ring(0xB1 + nvars, (4, 1 << nvars, D)), [(c[0], [0, 1]), (c[1], [1, 2]), (c[2], [3, 3]), (c[3], [2, 2, 2]), (c[4], [0])], 3


def shape_c(nvars):
    """the full envelope: 16 tables, 16 terms, a term with 8 factors, degree 8, term_off[q] = 64"""
    sizes = [8] + [4] * 11 + [3] * 4
    assert len(sizes) == 16 and sum(sizes) == 64
    c = rand_ring(0xC0 + nvars, (16, D))
    terms, k = [], 0
    for i, n in enumerate(sizes):
        terms.append((c[i], [(k + 5 * j) % 16 for j in range(n)]))
        k += 3
    return rand_ring(0xC1 + nvars, (16, 1 << nvars, D)), terms, 8


def shape_d(nvars):
    """claimed degree above the largest term: two factors at most, degree 5"""
    c = rand_ring(0xD0 + nvars, (2, D))
    return rand_ring(0xD1 + nvars, (3, 1 << nvars, D)), [(c[0], [0, 1]), (c[1], [2])], 5


def shape_e(nvars):
    """coefficients 0, 1, p - 1 (the +-1 shortcut and the zero term), a general one, and one that is 1 / p - 1 in a coefficient other than the constant"""
    g = rand_ring(0xE0 + nvars, (2, D))
    mixed = np.zeros(D, dtype=np.uint64)
    mixed[1], mixed[2] = 1, P - 1
    terms = [(_u64(const(0)), [0, 1]), (_u64(const(1)), [1, 2]), (_u64(const(P - 1)), [0, 2]), (g[0], [0]), (mixed, [2, 1, 0]), (g[1], [1, 1])]
    return rand_ring(0xE1 + nvars, (3, 1 << nvars, D)), terms, 3


def shape_f(nvars, mix):
    """reduction corners: every table word and coefficient word p - 1, or (mix) a pattern of 0 / 1 / p - 1 / (p - 1) / 2 / (p + 1) / 2"""
    n = 1 << nvars
    if mix:
        vals = np.array([0, 1, P - 1, (P - 1) // 2, (P + 1) // 2], dtype=np.uint64)
        tables = vals[(np.arange(3 * n * D) * 7 // 3) % 5].reshape(3, n, D)
        coef = vals[(np.arange(2 * D) * 3 + 2) % 5].reshape(2, D)
    else:
        tables = np.full((3, n, D), P - 1, dtype=np.uint64)
        coef = np.full((2, D), P - 1, dtype=np.uint64)
    return tables, [(coef[0], [0, 1, 2]), (coef[1], [0, 0])], 3


SHAPES = {"a": shape_a, "b": shape_b, "c": shape_c, "d": shape_d, "e": shape_e, "f-max": lambda nv: shape_f(nv, False), "f-mix": lambda nv: shape_f(nv, True)}
_PROOFS = {}


def case(shape, nvars):
    """(tables, terms, degree, msgs, point, final) of a named case on a fresh oracle transcript: computed once, shared, never written"""
    key = (shape, nvars)
    if key not in _PROOFS:
        tables, terms, degree = SHAPES[shape](nvars)
        out = (tables, terms, degree) + prove(lfp.Transcript(), tables, terms, degree)
        for a in (out[0],) + out[3:]:
            a.setflags(write=False)
        _PROOFS[key] = out
    return _PROOFS[key]
