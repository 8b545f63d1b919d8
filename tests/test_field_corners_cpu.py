"""CPU side of the reduction-corner tests (no GPU): the big-integer reference of tests/field_corners.py is pinned against the oracle on the very tables the GPU
tests feed, every GPU case is shown to reach every reduction corner (a condition on its inputs, so no GPU test can pass vacuously), and the host side of
lf_field.cuh runs against `unsigned __int128 %` under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import field_corners as fc
import lfo
from latticefold_amd.workload import RE

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "latticefold_amd", "csrc")
NU40 = 1 << 40


@pytest.fixture
def generic_oracle():
    """the oracle on F_p[Y]/(Y^3 - w^5) for the duration of a test"""
    nr, y = lfo.get_ring()
    nu2, y2 = fc.other_nonresidue()
    assert lfo.set_ring(nu2, y2) == 0
    yield nu2
    lfo.set_ring(nr, y.reshape(-1))


def _report(name, hits, allowed=()):
    """the coverage condition: every class at least once, except the documented ones"""
    print(f"{name:42s} " + " ".join(f"{k}={v}" for k, v in hits.items()))
    assert len(allowed) <= 2
    missing = [k for k, v in hits.items() if v == 0 and k not in allowed]
    assert not missing, f"{name}: the inputs never reach {missing}"


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def test_grid_and_tables():
    assert set(fc.EDGE_G) >= {0, 1, 2, fc.PG - 1, fc.PG - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**32 + 2, fc.PG - (2**32 - 1), 2**64 - 2**32, (fc.PG - 1) // 2,
                              (fc.PG + 1) // 2, 2**63, 2**63 + 1, 2**40, 2**24, fc.PG - 2**40, 0xFFFFFFFE00000001, 0xFFFFFFFEFFFFFFFF, 0x1FFFFFFFF, fc.PG - 2**32}      # every value the issue names
    for ring, p in (("goldilocks", fc.PG), ("babybear", fc.PB)):
        tau = 3 if ring == "goldilocks" else 9
        t = fc.corner_table(5, (40, 8 * tau), ring)
        assert (t < p).all() and fc.grid_share(t, ring) >= 0.5
        assert (t == fc.corner_table(5, (40, 8 * tau), ring)).all() and not (t == fc.corner_table(6, (40, 8 * tau), ring)).all()
        for q in range(tau):                              # grid words in every coordinate position
            assert fc.grid_share(t.reshape(-1, tau)[:, q], ring) >= 0.5
        A, B = fc.all_pairs(ring)
        a, b = A.reshape(-1, tau), B.reshape(-1, tau)
        g = fc.grid(ring)
        for i in range(tau):
            for j in range(tau):
                assert {(int(x), int(y)) for x, y in zip(a[:, i], b[:, j])} >= {(x, y) for x in g for y in g}


def test_grid_reaches_every_class_and_random_words_do_not():
    """the table of the issue: over grid x grid every F_p class occurs, over grid triples every F_{p^3} class; 3000 pseudo-random products take none of the
    rare ones (that is why the random-table parity tests cannot see a fault there)"""
    hits = dict.fromkeys(fc.FP_CLASSES, 0)
    for a in fc.EDGE_G:
        for b in fc.EDGE_G:
            for k in fc.classes_fp(a, b):
                hits[k] += 1
    print("grid x grid:", hits)
    assert all(hits.values())
    A, B = fc.all_pairs()
    pairs = list(zip(fc.exts(A.reshape(-1, 3)), fc.exts(B.reshape(-1, 3))))
    _report("all_pairs", fc.count_classes(pairs))
    w = fc.splitmix_fq(1, 0, 18000).reshape(-1, 2, 3)
    rnd = fc.count_classes([(tuple(int(v) for v in x), tuple(int(v) for v in y)) for x, y in w])
    print("3000 random products:", rnd)
    assert rnd["carry"] > 0 and all(rnd[k] == 0 for k in ("borrow", "hl0", "loose", "s128_up", "s128_down", "s128_loose"))


# ---- reference against oracle, and coverage, case by case ---------------------------------------------------------------------------------
def _logged(ref, fn, *a):
    ref.log = []
    out = fn(*a)
    pairs, ref.log = ref.log, None
    return out, pairs


@pytest.mark.parametrize("kind", fc.PRODUCT_KINDS)
def test_products(kind):
    wl, z = fc.products_case(kind)
    ref = fc.Ref()
    want, pairs = _logged(ref, ref.spmv, wl.rowptr[0], wl.col[0], fc.elems(wl.val[0]), fc.elems(z), wl.m)
    want = fc.pack(want)
    # oracle: slot-wise ring products, summed per row
    val, zz = np.ascontiguousarray(wl.val[0]), np.ascontiguousarray(z[wl.col[0]])
    prod = np.zeros_like(val)
    lfo.lib().lfo_ring_mul_ntt.argtypes = [lfo.u64p, lfo.u64p, lfo.u64p, lfo.C.c_size_t]
    lfo.lib().lfo_ring_mul_ntt(lfo._p64(val), lfo._p64(zz), lfo._p64(prod), val.shape[0])
    rp = wl.rowptr[0]
    for r in range(wl.m):
        acc = [0] * RE
        for k in range(int(rp[r]), int(rp[r + 1])):
            acc = [(x + int(y)) % fc.PG for x, y in zip(acc, prod[k])]
        assert [int(v) for v in want[r]] == acc, r
    nnz_per_row = int(rp[-1]) / min(wl.n, wl.m)
    assert (nnz_per_row > 1.5) == (kind == "rows")          # the dispatch rule of lf_ccs_load: more than 1.5 entries per row -> k_spmv_rows
    _report(f"products/{kind}", fc.count_classes(pairs))


@pytest.mark.parametrize("nv", fc.EQ_NVS)
def test_eq_and_mle(nv):
    """one GPU case per nv: its four points, both lengths, both tables.  Counted: the products the device forms (fc.eq_device_pairs: two half tables and an outer
    product from 6 variables on; one product per table entry, slot and eq entry for the evaluation)"""
    ref = fc.Ref()
    pairs = []
    for pk in fc.EQ_POINTS:
        pt = fc.point(pk, nv)
        eq, pp = fc.eq_device_pairs(ref, fc.exts(pt))
        pairs += pp
        assert eq == ref.eq_table(fc.exts(pt))
        assert (np.array(eq, dtype=np.uint64) == lfo.build_eq(fc.embed(pt))[:, 0:3]).all()
        for ln in sorted({1 << nv, max(1, (1 << nv) - 3)}):
            for t in fc.mle_tables(nv, ln):
                assert (fc.pack(ref.mle_eval(fc.elems(t), fc.exts(pt))) == lfo.mle_eval(t, fc.embed(pt))).all()
                pairs += fc.mle_device_pairs(fc.elems(t), eq)
    # The downward wrap of fq_from_s128 needs BOTH operands wholly on the grid (12 of the 1452 all_pairs products take it).  One variable: the eq entries r and
    # 1 - r are grid operands and meet the grid elements of the table -- all seven classes.  More variables: every eq entry is a product of at least five
    # factors, a generic field element, so these cases leave s128_down to the Products, lincomb and sumcheck cases.
    _report(f"eq+mle/nv{nv}", fc.count_classes(pairs, limit=None, distinct=True), allowed=() if nv == 1 else ("s128_down",))


@pytest.mark.parametrize("K,ln", fc.COMBINE_CASES)
def test_lincomb_and_horner(K, ln):
    ref = fc.Ref()
    coef, tabs = fc.lincomb_case(K, ln)
    want, pairs = _logged(ref, ref.lincomb, fc.elems(coef), fc.elems(tabs))
    assert (fc.pack(want) == lfo.lincomb(coef, tabs)).all()
    _report(f"lincomb/K{K}", fc.count_classes(pairs))
    tabs, ch = fc.horner_case(K, ln)
    want = ref.horner_combine(fc.elems(tabs), fc.exts(ch))
    assert (fc.pack(want) == lfo.horner_combine(tabs.reshape(2 * K, 3, ln, RE), fc.embed(ch))).all()
    _report(f"horner/K{K}", fc.count_classes(ref.horner_pairs(fc.elems(tabs), fc.exts(ch))))


def test_lin_rounds_reference_matches_oracle_proof():
    """the round-message reference replays a real linearization: tables M_j z, the oracle's beta and challenges -> the oracle's messages"""
    from latticefold_amd.workload import diag, make_workload
    for ccs in ("r1cs", "deg3"):
        wl = make_workload("T8", ccs=ccs)
        inst = lfo.Instance(wl)
        f = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([lfo.ajtai_commit(inst.ajtai_matrix(), wl.kappa, wl.N, lfo.crt(f)), wl.x_ccs])
        lc, pr = inst.linearize(lfo.Transcript(), cccs, f)
        tr = lfo.Transcript()
        tr.absorb_ring(diag(int.from_bytes(b"beta_s", "big") % fc.PG)[None, :])
        beta = [tuple(int(v) for v in tr.challenge()) for _ in range(wl.s)]
        ref = fc.Ref()
        z = fc.elems(wl.z())
        tabs = [ref.spmv(wl.rowptr[j], wl.col[j], fc.elems(wl.val[j]), z, wl.m) for j in range(wl.t)]
        msgs = ref.lin_rounds(tabs, beta, wl.S_off, wl.S_idx, fc.elems(wl.c), wl.d, fc.exts(lc[:wl.s, 0:3]))
        assert (fc.pack(msgs).reshape(-1, RE) == pr[:wl.s * (wl.d + 2)]).all(), ccs


@pytest.mark.parametrize("ccs,kind", fc.LIN_CASES)
def test_lin_round_coverage(ccs, kind):
    wl, tabs, beta, ch = fc.lin_case(ccs, kind)
    ref = fc.Ref()
    _, pairs = _logged(ref, ref.lin_rounds, fc.elems(tabs), fc.exts(beta), wl.S_off, wl.S_idx, fc.elems(wl.c), wl.d, fc.exts(ch))
    # counted over the products of whole grid operands (round 1's M_j M_k and eq M products at X = 0, 1).  A table of p - 1 alone has one first-level product,
    # (p-1, p-1, p-1)^2: it is there for the magnitude of the lazy sums, and leaves the two wraps it cannot produce to the "corner" tables
    if kind == "pm1":
        _report(f"lin/{ccs}/{kind}", fc.count_classes(pairs[:1500] + pairs[-1500:]), allowed=("s128_down", "s128_loose"))
    else:
        _report(f"lin/{ccs}/{kind}", fc.count_classes(pairs, grid_only=True))


def test_corner_witness_linearization_coverage():
    """test_linearization_of_a_corner_witness (GPU): beta and the challenges come from the transcript there, so only the products among the tables M_j z count
    -- grid elements of the witness met by grid elements (M_0 = M_1 = I) in round 1"""
    for ccs in ("r1cs", "deg3"):
        wl = fc.lin_witness_case(ccs)
        ref = fc.Ref()
        z = fc.elems(wl.z())
        tabs = [ref.spmv(wl.rowptr[j], wl.col[j], fc.elems(wl.val[j]), z, wl.m) for j in range(wl.t)]
        pairs = []
        for j in range(wl.t - 1):          # the first product of every term: M_j M_k at X = 0 and X = 1, every row and slot
            pairs += [(a, b) for x, y in zip(tabs[j], tabs[j + 1]) for a, b in zip(x, y)]
        _report(f"lin-witness/{ccs}", fc.count_classes(pairs, limit=None, grid_only=True, distinct=True))


@pytest.mark.parametrize("name,kind", fc.FOLD_CASES)
def test_fold_tables(name, kind):
    """the folding sumcheck's reference is the oracle (Instance.sumcheck_fold); what it shares with the big-integer code -- the eq tables, the ring product --
    is pinned above.  Here: the products round 1 forms on the device (fc.fold_round1_pairs; the eq tables are built on the host and uploaded, so their own
    products do not count) reach every corner"""
    wl, tabs, mu = fc.fold_case(name, kind)
    ref = fc.Ref()
    for idx, pt in zip((0, 2, 4), fc.fold_eq_points(wl, kind)):
        eq = ref.eq_table(fc.exts(pt))
        assert (np.array(eq, dtype=np.uint64) == lfo.build_eq(fc.embed(pt))[:, 0:3]).all()
        tabs[idx] = np.tile(np.array(eq, dtype=np.uint64), (1, 8))
    hits = fc.count_classes(fc.fold_round1_pairs(ref, wl, tabs, mu), limit=None, distinct=True)
    # Tables of p - 1 alone with b > 2: f-hat^2 is one product, mu meets the norm polynomial's value (a generic element), and the whole grid operands left are
    # eqR's r_0 and 1 - r_0 against G = (p-1, p-1, p-1) (fc.fold_eq_points): both wraps, but no loose result.  With b = 2 mu f-hat adds that.
    _report(f"fold/{name}/{kind}", hits, allowed=("s128_loose",) if (kind == "pm1" and wl.b > 2) else ())


def test_crt_reference_and_coverage():
    """CRT / ICRT as 24 x 24 matrices on big integers: inverse to each other, equal to the oracle on every row the GPU case feeds.  Coverage is counted for the
    dense ICRT (k_icrt_dense: 24-term sums in one Acc -- an F_p kernel: the classes of fq_from_s128 do not exist in it, Acc.ov != 0 takes their place, as for
    the generic non-residue) over the one GPU case, all four kinds of rows.  Its matrix entries are generic (multiples of 1/3), so a 24-term sum borrows with
    probability 2^-32 whatever the rows hold: left to the single products of the other cases.  The forward transform is a butterfly whose fq_mul operands are
    twiddles and intermediate sums, not input words: no predicate on the inputs describes them, so it has no entry; fq_mul itself is compared on grid x grid
    by lf_selftest_field."""
    F, I = fc.crt_matrices()
    assert all(sum(F[i][k] * I[k][j] for k in range(24)) % fc.PG == (i == j) for i in range(24) for j in range(24))
    rows = []
    for kind in fc.CRT_ROWS:
        for count in (1, 7, 257):
            x = fc.crt_rows(kind, count)
            g = fc.matvec(F, x)
            assert (g == lfo.crt(x)).all() and (fc.matvec(I, x) == lfo.icrt(x)).all() and (fc.matvec(I, g) == x).all()
            rows += list(x) + list(g)
    _report("icrt", fc.dense_rows_classes(I, rows), allowed=("borrow",))


@pytest.mark.parametrize("kind", fc.CRT_ROWS)
def test_crt_rows_roundtrip_on_the_oracle(kind):
    for count in (1, 7, 257):
        x = fc.crt_rows(kind, count)
        assert (lfo.icrt(lfo.crt(x)) == x).all() and (lfo.crt(lfo.icrt(x)) == x).all()


# ---- generic non-residue ------------------------------------------------------------------------------------------------------------
def test_generic_nonresidue_cases(generic_oracle):
    nu2 = generic_oracle
    ref = fc.Ref(nu=nu2)
    wl, z = fc.products_case("rows")
    want, pairs = _logged(ref, ref.spmv, wl.rowptr[0], wl.col[0], fc.elems(wl.val[0]), fc.elems(z), wl.m)
    val, zz = np.ascontiguousarray(wl.val[0]), np.ascontiguousarray(z[wl.col[0]])
    prod = np.zeros_like(val)
    lfo.lib().lfo_ring_mul_ntt.argtypes = [lfo.u64p, lfo.u64p, lfo.u64p, lfo.C.c_size_t]
    lfo.lib().lfo_ring_mul_ntt(lfo._p64(val), lfo._p64(zz), lfo._p64(prod), val.shape[0])
    assert (fc.pack(ref.rmul(fc.elems(val[5]), fc.elems(zz[5]))) == prod[5]).all() and (fc.pack(ref.rmul(fc.elems(val[100]), fc.elems(zz[100]))) == prod[100]).all()
    # the generic kernels never call fq_from_s128: its three classes give way to Acc.ov != 0 (a column sum of 2^128 or more)
    _report("generic/products", fc.count_classes(pairs, nu=nu2))
    pt = fc.point("grid", 7)
    t = fc.mle_tables(7, 125)[0]
    got, pairs = _logged(ref, ref.mle_eval, fc.elems(t), fc.exts(pt))
    assert (fc.pack(got) == lfo.mle_eval(t, fc.embed(pt))).all()
    _report("generic/eq+mle", fc.count_classes(pairs, nu=nu2))


# ---- the host program ------------------------------------------------------------------------------------------------------------------
def test_field_selftest_program_under_sanitizers():
    """make field-selftest: lf_field.cuh's host side against unsigned __int128 % over the grid, lazy sums up to the largest per-thread product count, under
    -fsanitize=address,undefined (a stand-alone program: nothing is loaded into this interpreter)"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "field-selftest"])
    r = subprocess.run([os.path.join(CSRC, "build", "lf_field_selftest")], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "selftest ok" in out and "runtime error" not in out and "Sanitizer" not in out
    assert "N_MAX = 65536" in out
    grid = [ln for ln in out.splitlines() if ln.strip().startswith("grid:")]
    assert [int(v, 16) for v in grid[0].split()[1:]] == fc.EDGE_G          # the program's copy of the grid is this module's


def test_the_three_copies_of_the_grid_agree():
    """EDGE_G here, GRID in lf_field_selftest.cpp (also printed by the program, above) and selftest::GRID in lf_capi.cpp (the device self-test's operands)"""
    import re
    for name, pname in (("lf_field_selftest.cpp", "P"), ("lf_capi.cpp", "PM")):
        with open(os.path.join(CSRC, name)) as f:
            body = re.search(r"\bGRID\[\w+\] = \{([^}]*)\}", f.read()).group(1)
        body = re.sub(r"(0x[0-9A-Fa-f]+|\d+)ULL", r"\1", body).replace("/", "//")
        vals = eval("[" + body + "]", {"__builtins__": {}}, {pname: fc.PG})
        assert vals == fc.EDGE_G, name
