"""The reference prover and verifier of the generic sumcheck tests (tests/test_mlsumcheck_cpu.py, tests/test_gpu_mlsumcheck.py): Python, none of it the code
under test.  Ring arithmetic is latticefold_amd.workload.ring_mul_ntt and modular numpy sums; Fiat-Shamir is the oracle's transcript (lfo.Transcript /
lfo_bb.Transcript).  The prover follows utils/sumcheck/prover.rs:111-143 literally -- per pair: the values at 0 and at 1, the step, repeated addition of the
step, the comb function at every point, the sum over the pairs -- and is NOT derived from the product's coefficients.  The verifier restates
verify_as_subprotocol (utils/sumcheck.rs:84-104, verifier.rs:92-257) with interpolate_uni_poly over F_{p^tau}.

A polynomial is a list of terms [(coef, [indices])], coef a ring element in NTT form ((RE,) uint64); tables are (T, n, RE)."""
import numpy as np

from latticefold_amd.workload import RINGS, _fp_add, diag, ring_mul_ntt


def oracle(ring):
    if ring == "goldilocks":
        import lfo
        return lfo
    import lfo_bb
    return lfo_bb


def rsub(a, b, ring):
    p = np.uint64(RINGS[ring][0])
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    with np.errstate(over="ignore"):
        return np.where(a >= b, a - b, a + (p - b))


def rsum(x, ring):
    """modular sum over the leading axis, pairwise"""
    x = np.asarray(x, dtype=np.uint64)
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        s = _fp_add(x[:h], x[h:2 * h], ring)
        x = s if x.shape[0] % 2 == 0 else np.concatenate([s, x[2 * h:]])
    return x[0]


def embed(r, ring):
    """a challenge (tau words) as a ring element: every slot carries it"""
    return np.tile(np.asarray(r, dtype=np.uint64), 8)


def comb(vals, terms, ring):
    """the comb function on (T, ..., RE) values: sum_i coef_i * prod_{k in indices_i} vals[k]"""
    acc = None
    for coef, idx in terms:
        pr = vals[idx[0]]
        for k in idx[1:]:
            pr = ring_mul_ntt(pr, vals[k], ring)
        pr = ring_mul_ntt(pr, np.asarray(coef, dtype=np.uint64), ring)
        acc = pr if acc is None else _fp_add(acc, pr, ring)
    return acc


def prove_round(tables, terms, degree, ring):
    """prover.rs:111-143 on the current tables (T, n, RE) -> (degree + 1, RE)"""
    v0, v1 = tables[:, 0::2], tables[:, 1::2]
    lev = [comb(v0, terms, ring), comb(v1, terms, ring)]
    steps, vals = rsub(v1, v0, ring), v1
    for _ in range(2, degree + 1):
        vals = _fp_add(vals, steps, ring)
        lev.append(comb(vals, terms, ring))
    return np.stack([rsum(l, ring) for l in lev[:degree + 1]])


def fix(tables, r, ring):
    """DenseMultilinearExtension::fix_variables of the lowest variable: new[j] = old[2j] + r (old[2j+1] - old[2j])"""
    v0, v1 = tables[:, 0::2], tables[:, 1::2]
    return _fp_add(v0, ring_mul_ntt(rsub(v1, v0, ring), embed(r, ring), ring), ring)


def prologue(tr, nvars, degree, ring):
    tr.absorb_ring(diag(nvars, ring))
    tr.absorb_ring(diag(degree, ring))


def transcript_round(tr, evals, ring):
    tr.absorb_ring(evals)
    r = tr.challenge()
    tr.absorb_ring(embed(r, ring))
    return r


def prove(tr, tables, terms, degree, ring):
    """prove_as_subprotocol on the oracle transcript `tr` -> (msgs (nvars, degree + 1, RE), point (nvars, tau), final (T, RE): the tables at the point)"""
    tables = np.asarray(tables, dtype=np.uint64)
    nvars = tables.shape[1].bit_length() - 1
    prologue(tr, nvars, degree, ring)
    msgs, point = [], []
    for _ in range(nvars):
        if point:
            tables = fix(tables, point[-1], ring)
        msgs.append(prove_round(tables, terms, degree, ring))
        point.append(transcript_round(tr, msgs[-1], ring))
    return np.stack(msgs), np.stack(point), fix(tables, point[-1], ring)[:, 0]


def hypercube_sum(tables, terms, ring):
    """sum of g over {0,1}^nvars, brute force"""
    return rsum(comb(np.asarray(tables, dtype=np.uint64), terms, ring), ring)


def ext_embed_int(v, ring):
    return diag(int(v) % RINGS[ring][0], ring)


def interpolate_uni_poly(p_i, at, ring):
    """sum_i p_i[i] prod_{j != i} (at - j) / (i - j) with `at` in F_{p^tau} (tau words) (verifier.rs:139-257, the plain Lagrange form)"""
    p = RINGS[ring][0]
    n = len(p_i)
    at_e = embed(at, ring)
    res = np.zeros(RINGS[ring][1], dtype=np.uint64)
    for i in range(n):
        num, den = ext_embed_int(1, ring), 1
        for j in range(n):
            if j != i:
                num = ring_mul_ntt(num, rsub(at_e, ext_embed_int(j, ring), ring), ring)
                den = den * (i - j) % p
        w = ring_mul_ntt(num, ext_embed_int(pow(den, p - 2, p), ring), ring)
        res = _fp_add(res, ring_mul_ntt(np.asarray(p_i[i], dtype=np.uint64), w, ring), ring)
    return res


def verify(tr, nvars, degree, claimed_sum, msgs, ring):
    """verify_as_subprotocol -> (ok, point, expected or the failing round): the transcript runs over every round first, the checks follow"""
    msgs = np.asarray(msgs, dtype=np.uint64).reshape(nvars, degree + 1, -1)
    prologue(tr, nvars, degree, ring)
    point = np.stack([transcript_round(tr, msgs[i], ring) for i in range(nvars)])
    expected = np.asarray(claimed_sum, dtype=np.uint64)
    for i in range(nvars):
        if not np.array_equal(_fp_add(msgs[i, 0], msgs[i, 1], ring), expected):
            return False, point, i
        expected = interpolate_uni_poly(msgs[i], point[i], ring)
    return True, point, expected


def g_at(final, terms, ring):
    """g evaluated on the tables' values at the point (T, RE)"""
    return comb(np.asarray(final, dtype=np.uint64), terms, ring)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def rand_ring(seed, shape, ring):
    from latticefold_amd.workload import splitmix_fq
    return splitmix_fq(seed, 0, int(np.prod(shape)), ring).reshape(shape)


def rand_poly(seed, nvars, ring, n_products=3, factors=(2, 5)):
    """the reference's rand_poly(nv, (2, 5), 3) shape (utils/sumcheck/utils.rs:186-230): n_products terms over DISJOINT tables, factors[0] .. factors[1]-1 factors
    each, a random coefficient each -> (tables, terms, degree)"""
    rng = np.random.default_rng(seed)
    terms, T = [], 0
    for i in range(n_products):
        k = int(rng.integers(factors[0], factors[1]))
        terms.append((rand_ring(seed * 131 + 7 * i + 1, (RINGS[ring][1],), ring), list(range(T, T + k))))
        T += k
    tables = rand_ring(seed * 977 + 5, (T, 1 << nvars, RINGS[ring][1]), ring)
    return tables, terms, max(len(ix) for _, ix in terms)


def _one(ring, v=1):
    return diag(v, ring)


def shape_a(nvars, ring):
    """the reference's own: rand_poly(nv, (2, 5), 3)"""
    return rand_poly(11 + nvars, nvars, ring)


def shape_b(nvars, ring):
    """sharing: two terms share table 1, a square, a cube, a single-factor term"""
    RE = RINGS[ring][1]
    c = rand_ring(0xB0 + nvars, (5, RE), ring)
    terms = [(c[0], [0, 1]), (c[1], [1, 2]), (c[2], [3, 3]), (c[3], [2, 2, 2]), (c[4], [0])]
    return rand_ring(0xB1 + nvars, (4, 1 << nvars, RE), ring), terms, 3


def shape_c(nvars, ring):
    """the full envelope: 16 tables, 16 terms, a term with 8 factors, degree 8, term_off[q] = 64"""
    RE = RINGS[ring][1]
    sizes = [8] + [4] * 11 + [3] * 4
    assert len(sizes) == 16 and sum(sizes) == 64
    c = rand_ring(0xC0 + nvars, (16, RE), ring)
    terms, k = [], 0
    for i, n in enumerate(sizes):
        terms.append((c[i], [(k + 5 * j) % 16 for j in range(n)]))
        k += 3
    return rand_ring(0xC1 + nvars, (16, 1 << nvars, RE), ring), terms, 8


def shape_d(nvars, ring):
    """claimed degree above the largest term: two factors at most, degree 5"""
    RE = RINGS[ring][1]
    c = rand_ring(0xD0 + nvars, (2, RE), ring)
    return rand_ring(0xD1 + nvars, (3, 1 << nvars, RE), ring), [(c[0], [0, 1]), (c[1], [2])], 5


def shape_e(nvars, ring):
    """coefficients 0, 1, p - 1 in every slot (the +-1 shortcut and the zero term), a general one, and one whose slots are of different classes"""
    p, RE, tau = RINGS[ring]
    g = rand_ring(0xE0 + nvars, (2, RE), ring)
    mixed = g[1].copy()
    mixed[0:tau] = 0
    mixed[tau:2 * tau] = 0
    mixed[tau] = 1
    mixed[2 * tau:3 * tau] = 0
    mixed[2 * tau] = p - 1
    terms = [(_one(ring, 0), [0, 1]), (_one(ring, 1), [1, 2]), (_one(ring, p - 1), [0, 2]), (g[0], [0]), (mixed, [2, 1, 0])]
    return rand_ring(0xE1 + nvars, (3, 1 << nvars, RE), ring), terms, 3


def shape_f(nvars, ring, mix):
    """reduction corners: every table word and coefficient word p - 1, or (mix) a pattern of 0 / 1 / p - 1 / (p - 1) / 2 / (p + 1) / 2"""
    p, RE, _tau = RINGS[ring]
    n = 1 << nvars
    if mix:
        vals = np.array([0, 1, p - 1, (p - 1) // 2, (p + 1) // 2], dtype=np.uint64)
        tables = vals[(np.arange(3 * n * RE) * 7 // 3) % 5].reshape(3, n, RE)
        coef = vals[(np.arange(2 * RE) * 3 + 2) % 5].reshape(2, RE)
    else:
        tables = np.full((3, n, RE), p - 1, dtype=np.uint64)
        coef = np.full((2, RE), p - 1, dtype=np.uint64)
    return tables, [(coef[0], [0, 1, 2]), (coef[1], [0, 0])], 3


SHAPES = {"a": shape_a, "b": shape_b, "c": shape_c, "d": shape_d, "e": shape_e,
          "f-max": lambda nv, ring: shape_f(nv, ring, False), "f-mix": lambda nv, ring: shape_f(nv, ring, True)}
_PROOFS = {}


def case(shape, nvars, ring):
    """(tables, terms, degree, msgs, point, final) of a named case on a fresh oracle transcript: computed once, shared, never written"""
    key = (shape, nvars, ring)
    if key not in _PROOFS:
        tables, terms, degree = SHAPES[shape](nvars, ring)
        out = (tables, terms, degree) + prove(oracle(ring).Transcript(), tables, terms, degree, ring)
        for a in (out[0],) + out[3:]:
            a.setflags(write=False)
        _PROOFS[key] = out
    return _PROOFS[key]
