"""The Frog-ring corner cases on the CPU: the Python-integer reference of tests/lfp_field_corners.py against the oracle (tests/lfp.py) on the very tables
tests/test_gpu_lfp_field_corners.py feeds the device, and the proof that those tables reach the rare branches of latticefold_amd/csrc/lfp_field.cuh.

The proof runs the branch model (fc.Dev and fc.dev_*: the kernels' use of mont_mul, add_p, sub_p and the lazy 160-bit sums restated call by call on Python
integers) over every case and asserts, corner by corner, that a NAMED case reaches it -- an edit to a case that loses its corner fails here, without a GPU.  The
model is also held to the reference: what it computes along the way is the reference's result, so it cannot drift from the arithmetic it describes.  It is never
the source of an expected value of the GPU tests."""
import numpy as np
import pytest

import lfp
import lfp_field_corners as fc
import lfplus_mlsumcheck_ref as ref

P, D = fc.P, fc.D


# ---- the reference against the oracle -------------------------------------------------------------------------------------------------------------------------
def test_scalar_products_match_the_oracle():
    assert np.array_equal(fc.tensor_product(fc.GRID, fc.GRID), lfp.tensor_product(fc.GRID, fc.GRID))
    assert np.array_equal(fc.tensor_product(fc.PAIR_A, fc.PAIR_B), lfp.tensor_product(fc.PAIR_A, fc.PAIR_B))
    for name, r in fc.TENSOR_POINTS.items():
        assert np.array_equal(fc.tensor(r), lfp.tensor(r)), name


@pytest.mark.parametrize("name", sorted(fc.ring_mul_cases()))
def test_ring_products_match_the_oracle(name):
    a, b, broadcast = fc.ring_mul_cases()[name]
    want = np.zeros(a.shape[1:], dtype=np.uint64)
    for i in range(a.shape[0]):
        for x in range(a.shape[1]):
            want[x] = lfp.addmod(want[x], lfp.ring_mul(a[i, x], b[i] if broadcast else b[i, x]))
    assert np.array_equal(fc.ring_mul_sum(a, b, broadcast), want)


def test_matrix_products_match_the_oracle():
    mats, x = fc.spmv_case()
    for j, m in enumerate(mats):
        assert np.array_equal(fc.spmv(m, x), ref.spmv(m, x)), j                     # (ref.spmv: the oracle's ring product, summed in Python)
    # one dense row of ring coefficients is a commitment with kappa = 1
    A = fc.rows_u64([fc.grid_row(3 * j + 1, 2) for j in range(x.shape[0])])
    row = (np.array([0, x.shape[0]], dtype=np.uint32), np.arange(x.shape[0], dtype=np.uint32), A)
    assert np.array_equal(fc.spmv(row, x), lfp.commit(A[None], x))


@pytest.mark.parametrize("name", sorted(fc.SHAPES))
def test_planted_instances_are_satisfied_by_the_oracle(name):
    """the product rows planted in the witnesses of the relation checks and of the linearization, recomputed with the oracle's ring product"""
    cases = [fc.check_case(name)[:2]] + [fc.lin_case(name, nv) for nv in (4, 5)]
    for mats, f in cases:
        ga, gb, gc = (ref.spmv(m, f) for m in mats)
        for r in range(f.shape[0]):
            pr = lfp.ring_mul(ga[r], gb[r])
            if name == "deg3":
                c = np.zeros(D, dtype=np.uint64)
                c[0] = fc.CCS_CONST
                pr = lfp.ring_mul(lfp.ring_mul(pr, gb[r]), c)
            assert np.array_equal(pr, gc[r]), (name, r)


@pytest.mark.parametrize("B", fc.DECOMP_BASES)
def test_balanced_digits_match_the_oracle(B):
    f, corners = fc.decompose_f(B)
    n = f.shape[0]
    A = ref.rand_ring(0xDC + B % 97, (1, n, D))
    r = np.zeros((10, D), dtype=np.uint64)
    want = lfp.decompose(f, A, B, r, r)
    F0, F1 = fc.decompose2(f, B)
    assert np.array_equal(F0, want["F0"]) and np.array_equal(F1, want["F1"])
    ok, fits = fc.decompose_identities(f, F0, F1, B)
    assert ok and fits > 0.9 * f.size                        # (the planted (p +- 1) / 2 do not fit two digits of a small base: their third digit is dropped)
    assert all(c % P in set(int(w) for w in f.reshape(-1)) for c in corners)


def test_evaluations_match_the_oracle():
    """fc.mle_const (the evaluations linb_check is given) against the oracle's decompose with B = 2^62, which leaves F0 = f and returns mle(f)(r), mle(M f)(r)"""
    f, r, mats, v = fc.linb_case()
    A = ref.rand_ring(0x11B, (1, f.shape[0], D))
    dec = lfp.decompose(f, A, 1 << 62, np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1]), mats)
    small = np.vectorize(lambda w: abs(fc.centre(w)) < 1 << 61)(f)
    if small.all():                                           # (B = 2^62 leaves F0 = f only for such words; the grid has larger ones)
        assert np.array_equal(dec["v0"], v)
    fs = np.where(small, f, np.uint64(1))
    Mfs = (fs.astype(object) * mats[0][2][:, :1].astype(object) % P).astype(np.uint64)
    dec = lfp.decompose(fs, A, 1 << 62, np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1]), mats)
    assert np.array_equal(dec["F0"], fs)
    want = np.stack([np.stack([fc.mle_const(t, r[:, pt, 0]) for pt in range(2)]) for t in (fs, Mfs)])
    assert np.array_equal(dec["v0"], want)


# ---- the branch model over every case ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """one fc.Dev that has run every modelled GPU case under its name; along the way the model's results are the reference's"""
    d = fc.Dev()
    d.case = "tensor_product/grid"
    assert fc.dev_tensor_product(d, fc.GRID, fc.GRID) == fc.tensor_product(fc.GRID, fc.GRID).tolist()
    d.case = "tensor_product/pairs"
    assert fc.dev_tensor_product(d, fc.PAIR_A, fc.PAIR_B) == fc.tensor_product(fc.PAIR_A, fc.PAIR_B).tolist()
    for name, r in fc.TENSOR_POINTS.items():
        d.case = "tensor/" + name
        assert fc.dev_tensor(d, r) == fc.tensor(r).tolist()
    for name, (a, b, broadcast) in fc.ring_mul_cases().items():
        d.case = "ring_mul/" + name
        assert fc.dev_ring_mul(d, a, b, broadcast) == fc.ring_mul_sum(a, b, broadcast).tolist(), name
    mats, x = fc.spmv_case()
    for j, m in enumerate(mats):
        d.case = ("spmv/ring", "spmv/const", "spmv/ones")[j]
        assert fc.dev_spmv(d, m, x) == fc.spmv(m, x).tolist()
    for nv in fc.MLS_NVARS:
        d.case = f"mlsumcheck/nvars{nv}"
        tables, terms, degree, ch = fc.mls_case(nv)
        msgs, fin = fc.dev_mls(d, tables, terms, degree, ch)
        T, rt = tables.astype(object), ref.terms_as_rings(terms)
        for rnd in range(nv):
            if rnd:
                T = ref.fix(T, ch[rnd - 1])
            assert (ref.prove_round(T, rt, degree) == np.array(msgs[rnd], dtype=object)).all(), (nv, rnd)
        assert (ref.fix(T, ch[nv - 1])[:, 0] == np.array(fin, dtype=object)).all()
    mats, f, _ = fc.check_case("r1cs")
    d.case = "r1cs_check"
    assert fc.dev_r1cs_residual(d, mats, f) == []
    return d


def _need(model, label, *cases):
    for case in cases:
        assert model.supplied(label, case), f"{case} no longer reaches {label!r}; it is reached by {sorted(model.hits.get(label, ()))}"


def test_mont_mul_classes_are_reached(model):
    """(cy, o1, o2, v >= p): the three classes random operands reach, cy = 0 with a non-zero product, o2 = 1"""
    for cls in fc.MONT_COMMON:
        _need(model, ("mont",) + cls, "tensor_product/grid", "tensor_product/pairs")
    _need(model, "mont cy0 nonzero", "tensor_product/pairs", "tensor_product/grid", "spmv/const", "mlsumcheck/nvars4", "mlsumcheck/nvars5", "tensor/len6")
    _need(model, ("mont", 1, 0, 1, 0), "tensor_product/pairs", "spmv/const")
    assert not [k for k in model.hits if isinstance(k, tuple) and k[3] and (k[2] or k[4])], "o2 = 1 leaves v = 0: it never meets o1 or v >= p"


def test_mont_mul_boundaries_are_reached(model):
    for name in fc.VFULL_BOUNDS.values():
        _need(model, "vfull " + name, "tensor_product/pairs", "spmv/const")
    for name in ("p-1", "p+1"):                                   # the conversions: to_mont of the operands computed for these two
        _need(model, "vfull " + name, "tensor/len6", "mlsumcheck/nvars5")


def test_add_and_sub_branches_and_corners_are_reached(model):
    for label in ("add none", "add ge", "add wrap", "add =p", "add =p-1", "add =2^64-1", "add =2^64"):
        _need(model, label, "spmv/ones")
    for label in ("sub ge", "sub lt", "sub a=b", "sub 0-(p-1)", "sub a=b-1"):
        _need(model, label, "mlsumcheck/nvars1", "mlsumcheck/nvars4", "mlsumcheck/nvars5")


def test_signed_lazy_sums_reach_their_corners(model):
    for k in (1, 2, 3, 4):
        _need(model, f"s neg zl{k}", "ring_mul/sign chain")
    _need(model, "s neg zl3", "mlsumcheck/nvars4")
    _need(model, "s pos zl", "ring_mul/sign chain", "ring_mul/mono0/count17")
    _need(model, "s borrow5", "ring_mul/mono15/count33", "ring_mul/pairs X^15", "mlsumcheck/nvars4", "r1cs_check")
    _need(model, "s carry5", "ring_mul/mono0/count17", "ring_mul/terms2/count33", "mlsumcheck/nvars4", "r1cs_check")
    for w in ("00", "01", "10", "11"):
        _need(model, "s w" + w, "ring_mul/mono15/count33", "ring_mul/terms2/count33", "mlsumcheck/nvars4", "r1cs_check")
    for label in ("s w4 below", "s w4 notbelow"):
        _need(model, label, "ring_mul/mono15/count33", "ring_mul/terms3/count17/broadcast", "mlsumcheck/nvars1", "r1cs_check")
    # w1 in [p, 2^64) alone does not show a missing reduction (add_p absorbs most of it): these cases hold constructed sums for which acc160_red returns
    # another word (the right one plus p) without it.  k_r1cs_residual compares that word at once (row 16 of the instance); the sumcheck adds it to 0 first.
    # The reduction of w0 never matters: mont_mul(w0, 1) is right for every 64-bit w0
    _need(model, "s w1 reduction needed", "mlsumcheck/nvars1", "mlsumcheck/nvars4", "mlsumcheck/nvars5", "r1cs_check")
    assert not model.supplied("s w0 reduction needed") and not model.supplied("u w0 reduction needed")


def test_unsigned_lazy_sums_reach_their_corners(model):
    for label in ("u carry5", "u w00", "u w01", "u w10", "u w11", "u mult p"):
        _need(model, label, "r1cs_check")


def test_accepted_rows_carry_the_constructed_products():
    """row r < len(PAIRS) of the relation-check instance: g_A is the canonical value of the pair's first word (its to_mont is the word), lane r of g_B the
    second word, so coefficient r of the row's product holds first x second as a term"""
    for name in fc.SHAPES:
        mats, f, rows = fc.check_case(name)
        ga, gb = fc.spmv(mats[0], f), fc.spmv(mats[1], f)
        for pair, r in rows.items():
            a, b = fc.PAIRS[pair]
            assert fc.word_of(int(ga[r, 0])) == a and not ga[r, 1:].any() and int(gb[r, r]) == b, (name, pair)
        assert {"o2 issue", "vfull 2^64", "cy0 2^32 2^32", "vfull p-1", "vfull p+1", "vfull 2^64-1", "vfull 2^64+1"} <= set(rows)


# ---- the blind spot ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_canonical_corners_of_the_existing_tests_reach_neither_rare_class():
    """edge_rows() of test_gpu_lfplus_ring_ops.py (pairwise, both modes) and shape_f of lfplus_mlsumcheck_ref.py (all p - 1, and the 0 / 1 / p - 1 / (p +- 1) / 2
    pattern; the challenges are the transcript's) through the same model: no cy = 0 with a non-zero product, no o2 = 1, none of the upper three boundaries"""
    import test_gpu_lfplus_ring_ops as ring_ops
    d = fc.Dev()
    e = ring_ops.edge_rows()
    d.case = "edge_rows"
    a, b = np.repeat(e, 5, axis=0), np.tile(e, (5, 1))
    assert fc.dev_ring_mul(d, a[None], b[None], False) == fc.ring_mul_sum(a[None], b[None], False).tolist()
    for i in range(5):
        fc.dev_ring_mul(d, e[None], e[i][None], True)
    for shape in ("f-max", "f-mix"):
        for nv in (1, 2, 4, 5):
            tables, terms, degree, msgs, point, final = ref.case(shape, nv)
            d.case = f"{shape}/{nv}"
            m, fin = fc.dev_mls(d, tables, terms, degree, point)
            assert (np.array(m, dtype=object) == msgs.astype(object)).all() and (np.array(fin, dtype=object) == final.astype(object)).all()
    assert ("mont", 1, 0, 0, 0) in d.hits and "s w00" in d.hits
    assert not d.supplied("mont cy0 nonzero") and not d.supplied(("mont", 1, 0, 1, 0))
    assert not any(d.supplied("vfull " + n) for n in ("2^64-1", "2^64", "2^64+1"))
