"""CPU side of the BabyBear device-word corner tests (no GPU).  The BabyBear kernels work on centred Montgomery words in [-H, H] (bb_field.cuh); the corner grid
of tests/field_corners.py for this ring, EDGE_BW, is therefore a grid of DEVICE words.  Here the big-integer reference is pinned against the BabyBear oracle on
the very tables tests/test_gpu_bb_field_corners.py feeds, every GPU case is shown -- from the operand pairs the device forms -- to reach the branches of mred, the
top of the 64-bit column, the 96-bit lazy sums past 2^64 and the +-128 digits of the int8 paths (a condition on the inputs, so no GPU test can pass vacuously),
the canonical grid EDGE_B is shown to reach none of them, and the host side of bb_field.cuh runs against plain `%` under the address and undefined-behaviour
sanitizers as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_corners as fc
import lfo_bb
from field_corners import BB

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "latticefold_amd", "csrc")
TOP = ("pre_up", "pre_down", "col_top")


@pytest.fixture
def generic_oracle():
    """the BabyBear oracle on F_p[Y]/(Y^9 - zeta) for the duration of a test"""
    nr, y = lfo_bb.get_ring()
    nu2, y2 = fc.other_nonresidue_bb()
    assert lfo_bb.set_ring(nu2, y2) == 0
    yield nu2
    lfo_bb.set_ring(nr, y.reshape(-1))


def _report(name, hits, allowed=()):
    """the coverage condition: every class at least once, except the documented ones"""
    print(f"{name:34s} " + " ".join(f"{k}={v}" for k, v in hits.items()))
    missing = [k for k, v in hits.items() if v == 0 and k not in allowed]
    assert not missing, f"{name}: the inputs never reach {missing}"


def _logged(ref, fn, *a):
    ref.log = []
    out = fn(*a)
    pairs, ref.log = ref.log, None
    return out, pairs


def _pairs_of(A, B):
    return list(zip(fc.exts(A.reshape(-1, 9)), fc.exts(B.reshape(-1, 9))))


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def test_word_grid_and_tables():
    H, R = fc.HB, fc.RB
    assert H == 0x3C000000 and R == 2**32 % fc.PB and fc.canon(R) == 1 and fc.canon(-R) == fc.PB - 1
    need = [0, 1, -1, 2, -2, H, -H, H - 1, 1 - H, H // 2, -(H // 2), H // 2 + 1, -(H // 2) - 1, R, -R, 2**29, -2**29, 0x3B7F7F7F, -0x3B7F7F7F, 0x3B808080, -0x3B808080,
            0x007F7F7F, -0x00808080, 0x7F, -0x80, 0x80, -0x81, 0x7FFF, 0x8000, -0x8000]                    # every word the issue names
    assert set(fc.EDGE_BW) >= set(need) and all(-H <= w <= H for w in fc.EDGE_BW)
    assert all(fc.word(fc.canon(w)) == w and fc.canon(w) == w * pow(2, -32, fc.PB) % fc.PB for w in fc.EDGE_BW)
    assert [fc.digits_bb(w)[0] for w in (0x3B7F7F7F, 0x3B808080, -0x3B808080)] == [[127, 127, 127, 59], [-128, -127, -127, 60], [-128, -128, -128, -59]]
    # existing callers see the canonical grid and unchanged tables
    assert fc.grid(BB) is fc.EDGE_B and fc.grid() is fc.EDGE_G and fc.grid_share(fc.corner_table(5, (40, 72), BB), BB) >= 0.5
    t = fc.corner_table(5, (40, 72), BB, words=True)
    assert (t < fc.PB).all() and fc.grid_share(t, BB, words=True) >= 0.5 and not (t == fc.corner_table(5, (40, 72), BB)).all()
    for q in range(9):
        assert fc.grid_share(t.reshape(-1, 9)[:, q], BB, words=True) >= 0.5
    for rot in (None, fc.BB_ROTATIONS):
        A, B = fc.all_pairs(BB, words=True, rotations=rot, sat_nus=(2,))
        a, b = A.reshape(-1, 9), B.reshape(-1, 9)
        assert fc.exts(a[:18]) == [x for x, _ in fc.saturating_pairs()] and fc.exts(b[:18]) == [y for _, y in fc.saturating_pairs()]      # in front
        g = fc.EDGE_BWC
        for i in range(9):
            for j in range(9):
                assert {(int(x), int(y)) for x, y in zip(a[:, i], b[:, j])} >= {(x, y) for x in g for y in g}
    for nu in (2, fc.other_nonresidue_bb()[0]):              # column k of saturating pair k is nine terms of +-H^2
        for idx, (a, b) in enumerate(fc.saturating_pairs(nu)):
            assert fc.bb_columns(a, b, nu)[1][idx % 9] == (1 if idx < 9 else -1) * 9 * H * H
    assert (fc.table("wmax", 0, (3, 72), BB) == fc.canon(H)).all() and (fc.table("wmin", 0, (3, 72), BB) == fc.canon(-H)).all()
    assert fc.canon(H) == 1541406721 and fc.canon(-H) == 471859200


def test_the_canonical_grid_reaches_none_of_these_branches():
    """why the word grid exists (the table of the issue, recomputed): over EDGE_B x EDGE_B in every position, and over the all-(p - 1) / all-(p +- 1) / 2 operands
    of the ring-product and sumcheck tests, no column's high half exceeds H before mred centres it and no column comes near the top of its register; the
    word grid with the saturating pairs reaches both, the k = 8 pair alone already does"""
    A, B = fc.all_pairs(BB)
    old = _pairs_of(A, B)
    named = [(fc.PB - 1,) * 9, ((fc.PB - 1) // 2,) * 9, ((fc.PB + 1) // 2,) * 9]
    old += [(x, y) for x in named for y in named]
    hits = fc.count_classes_bb(old)
    print("EDGE_B:", hits)
    assert all(hits[k] == 0 for k in TOP)
    for v, frac in ((fc.PB - 1, -0.267), ((fc.PB - 1) // 2, -0.133), ((fc.PB + 1) // 2, 0.133)):
        assert abs(fc.word(v) / fc.HB - frac) < 1e-3
    top = lambda prs: max(abs(T) for a, b in prs for T in fc.bb_columns(a, b)[1]) / 2.0**63
    hi = lambda prs: max(abs(T >> 32) for a, b in prs for T in fc.bb_columns(a, b)[1]) / fc.HB
    print(f"largest column / high half: EDGE_B {top(old):.3f} 2^63, {hi(old):.2f} H; p - 1 alone {top([(named[0], named[0])]):.3f} 2^63")
    assert top(old) < 0.5 and hi(old) <= 1
    for x, t63, th in ((named[0], 0.133, 0.28), (named[1], 0.033, 0.07), (named[2], 0.033, 0.07)):      # the rows of the table in DESIGN.md
        assert abs(top([(x, x)]) - t63) < 1e-3 and abs(hi([(x, x)]) - th) < 6e-3
    sat = fc.saturating_pairs()
    assert abs(top(sat) - 0.98877) < 1e-5 and abs(hi(sat) - 2.11) < 0.01
    k8 = fc.count_classes_bb([sat[8], sat[17]])
    assert k8["col_top"] and k8["pre_up"] and k8["pre_down"]
    A, B = fc.all_pairs(BB, words=True, sat_nus=(2,))
    _report("word grid all_pairs", fc.count_classes_bb(_pairs_of(A, B)))
    w = fc.splitmix_fq(1, 0, 18 * 3000, BB).reshape(-1, 2, 9)
    rnd = fc.count_classes_bb([(tuple(int(v) for v in x), tuple(int(v) for v in y)) for x, y in w])
    print("3000 random products:", rnd)
    assert rnd["col_top"] == 0 and rnd["pre_up"] + rnd["pre_down"] < 30


# ---- reference against oracle, and coverage, case by case ---------------------------------------------------------------------------------
def _oracle_products(val, zz):
    prod = np.zeros_like(val)
    lfo_bb.lib().lfo_ring_mul_ntt.argtypes = [lfo_bb.u64p, lfo_bb.u64p, lfo_bb.u64p, lfo_bb.C.c_size_t]
    lfo_bb.lib().lfo_ring_mul_ntt(lfo_bb._p64(val), lfo_bb._p64(zz), lfo_bb._p64(prod), val.shape[0])
    return prod


def _products(kind, nu):
    wl, z = fc.products_case_bb(kind)
    ref = fc.Ref(BB, nu=nu)
    want, pairs = _logged(ref, ref.spmv, wl.rowptr[0], wl.col[0], fc.elems(wl.val[0], BB), fc.elems(z, BB), wl.m)
    want = fc.pack(want)
    val, zz = np.ascontiguousarray(wl.val[0]), np.ascontiguousarray(z[wl.col[0]])
    prod = _oracle_products(val, zz)
    rp = wl.rowptr[0]
    for r in range(wl.m):
        acc = prod[int(rp[r]):int(rp[r + 1])].astype(object).sum(axis=0) % fc.PB if rp[r + 1] > rp[r] else np.zeros(72, dtype=object)
        assert [int(v) for v in want[r]] == [int(v) for v in acc], r
    # k_spmv multiplies e9_mul(val, z): the logged (val, z) pairs are the device's, z the pre-multiplied operand
    return fc.count_classes_bb(pairs, nu=2 if nu is None else nu)


@pytest.mark.parametrize("kind", fc.PRODUCT_KINDS)
def test_products(kind):
    _report(f"products/{kind}", _products(kind, None))


def test_products_generic_nonresidue(generic_oracle):
    _report("products/rows/generic", _products("rows", generic_oracle))


@pytest.mark.parametrize("nv", fc.EQ_NVS)
def test_eq_and_mle(nv):
    """one GPU case per nv: its four points, both lengths, both tables.  k_build_eq forms every entry as the running product of its nv factors (the pairs of the
    doubling recursion), k_dot_eq one product e9_mul(table element, eq entry) per entry and slot"""
    ref = fc.Ref(BB)
    pairs = []
    for pk in fc.EQ_POINTS_BB:
        pt = fc.point(pk, nv, BB, words=True)
        eq, pp = fc.eq_device_pairs(ref, fc.exts(pt))
        pairs += pp
        assert (np.array(eq, dtype=np.uint64) == lfo_bb.build_eq(fc.embed(pt, BB))[:, 0:9]).all()
        for ln in sorted({1 << nv, max(1, (1 << nv) - 3)}):
            for t in fc.mle_tables_bb(nv, ln):
                assert (fc.pack(ref.mle_eval(fc.elems(t, BB), fc.exts(pt))) == lfo_bb.mle_eval(t, fc.embed(pt, BB))).all()
                pairs += fc.mle_device_pairs(fc.elems(t, BB), eq)
    _report(f"eq+mle/nv{nv}", fc.count_classes_bb(pairs))


@pytest.mark.parametrize("K,ln", fc.COMBINE_CASES)
def test_lincomb_and_horner(K, ln):
    """one GPU case per (K, ln), its three kinds of operands together.  k_lincomb_z adds the un-reduced columns of its 2K (lincomb) / 6K (horner_combine)
    products e9_mul_cols(table element, coefficient) in 96-bit sums: of the product classes the size of the column and the doubling are the kernel's, the
    reduction is hl_finish's.  Counted over the first rows (the tables repeat with period two)."""
    ref = fc.Ref(BB)
    tot = {}
    for kind in fc.COMBINE_KINDS_BB:
        coef, tabs = fc.lincomb_case_bb(K, ln, kind)
        assert (fc.pack(ref.lincomb(fc.elems(coef, BB), fc.elems(tabs, BB))) == lfo_bb.lincomb(coef, tabs)).all()
        tabs_h, ch = fc.horner_case_bb(K, ln, kind)
        assert (fc.pack(ref.horner_combine(fc.elems(tabs_h, BB), fc.exts(ch))) == lfo_bb.horner_combine(tabs_h, fc.embed(ch, BB))).all()
        for what, sums in (("lincomb", fc.lincomb_device_sums(coef, tabs, rows=min(ln, 8))), ("horner", fc.horner_device_sums(ref, tabs_h, ch, rows=min(ln, 4)))):
            mul = fc.count_classes_bb([p for s in sums for p in s])
            hits = {k: mul[k] for k in ("col_top", "dbl_wrap")} | fc.count_classes_hl(sums)
            print(f"{what}/K{K}/{kind:24s} " + " ".join(f"{k}={v}" for k, v in hits.items()))
            if kind == "wsat":
                assert hits["hl_a2_pos"] and hits["hl_a2_neg"] and hits["col_top"]      # 2K saturated columns: the sum passes 2^64 in both directions
            for k, v in hits.items():
                tot[what, k] = tot.get((what, k), 0) + v
    _report(f"lincomb+horner/K{K}", tot)


def test_lin_rounds_reference_matches_oracle_proof():
    """the round-message reference replays a real BabyBear linearization: tables M_j z, the oracle's beta and challenges -> the oracle's messages"""
    from latticefold_amd.workload import diag, make_workload
    for ccs in ("r1cs", "deg3"):
        wl = make_workload("B6", ccs=ccs)
        inst = lfo_bb.Instance(wl)
        f = inst.witness_from_w_ccs(wl.w_ccs)
        cccs = np.concatenate([lfo_bb.ajtai_commit(inst.ajtai_matrix(), wl.kappa, wl.N, lfo_bb.crt(f)), wl.x_ccs])
        lc, pr = inst.linearize(lfo_bb.Transcript(), cccs, f)
        tr = lfo_bb.Transcript()
        tr.absorb_ring(diag(int.from_bytes(b"beta_s", "big") % fc.PB, BB)[None, :])
        beta = [tuple(int(v) for v in tr.challenge()) for _ in range(wl.s)]
        ref = fc.Ref(BB)
        z = fc.elems(wl.z(), BB)
        tabs = [ref.spmv(wl.rowptr[j], wl.col[j], fc.elems(wl.val[j], BB), z, wl.m) for j in range(wl.t)]
        msgs = ref.lin_rounds(tabs, beta, wl.S_off, wl.S_idx, fc.elems(wl.c, BB), wl.d, fc.exts(lc[:wl.s, 0:9]))
        assert (fc.pack(msgs).reshape(-1, 72) == pr[:wl.s * (wl.d + 2)]).all(), ccs


@pytest.mark.parametrize("ccs,kind", fc.LIN_CASES_BB)
def test_lin_round_coverage(ccs, kind):
    """counted over the products of two whole table elements: round 1's M_0 M_1 at X = 0 and X = 1, which the device forms as e9_mul(M_0, M_1) (k_lin_round,
    k_lin_r1cs, k_lin_small: the term starts at its first table and is multiplied by the next; the constant c_0 = 1 of the reference's first product changes
    nothing) -- M_1 is the pre-multiplied operand on both sides"""
    wl, tabs, beta, ch = fc.lin_case_bb(ccs, kind)
    ref = fc.Ref(BB)
    assert fc.elems(np.asarray(wl.c).reshape(-1, 72)[0], BB) == [ref.one] * 8
    _, pairs = _logged(ref, ref.lin_rounds, fc.elems(tabs, BB), fc.exts(beta), wl.S_off, wl.S_idx, fc.elems(wl.c, BB), wl.d, fc.exts(ch))
    els = {sl for t in fc.elems(tabs, BB) for x in t for sl in x}
    hits = fc.count_classes_bb(pairs, only=els)
    # tables of +H alone multiply to +9 H^2 only (the negative column is the "wsat" case's); the saturating pattern has no word whose double wraps
    _report(f"lin/{ccs}/{kind}", hits, allowed={"corner": (), "wmax": ("pre_down", "post_up", "post_down", "dbl_wrap", "canon_neg"), "wsat": ("dbl_wrap",)}[kind])
    assert kind == "corner" or hits["col_top"]


@pytest.mark.parametrize("name,kind", fc.FOLD_CASES_BB)
def test_fold_tables(name, kind):
    """the folding sumcheck's reference is the oracle; the eq tables the GPU test uploads are the big-integer ones, pinned here.  Coverage: the products round 1
    forms for its first pairs (fc.fold_round1_pairs, b = 2: f^2, mu f, the lazy (mu f) f^2 products, eq x G).  The 96-bit sums of k_fold_round are not
    counted: at these sizes the launcher splits the 2K * 9 tables over 32 chunks, nine derived products (mu f) (f^2 - 1) per sum, which no choice of tables
    drives past 2^64 -- the top word of hl_finish is lincomb's and horner_combine's to test"""
    wl, tabs, mu = fc.fold_case_bb(name, kind)
    ref = fc.Ref(BB)
    for idx, pt in zip((0, 2, 4), fc.fold_eq_points_bb(wl, kind)):
        eq = ref.eq_table(fc.exts(pt))
        assert (np.array(eq, dtype=np.uint64) == lfo_bb.build_eq(fc.embed(pt, BB))[:, 0:9]).all()
        tabs[idx] = np.tile(np.array(eq, dtype=np.uint64), (1, 8))
    hits = fc.count_classes_bb(fc.fold_round1_pairs(ref, wl, tabs, mu))
    _report(f"fold/{name}/{kind}", hits)


def test_crt_reference_and_coverage():
    """CRT / ICRT as 72 x 72 matrices on big integers: inverse to each other, equal to the oracle on every row the GPU case feeds.  k_icrt_dense reduces eight
    nine-term groups per output word: the "wsat" rows give every product of one output the sign of its matrix entry, the largest group that matrix allows"""
    F, I = fc.crt_matrices_bb()
    Fn, In = np.array(F, dtype=object), np.array(I, dtype=object)
    assert ((Fn.dot(In) % fc.PB) == np.eye(72, dtype=object)).all()
    rows = []
    for kind in fc.CRT_ROWS_BB:
        for count in fc.CRT_COUNTS_BB:
            x = fc.crt_rows_bb(kind, count, I)
            g = fc.matvec_bb(F, x)
            assert (g == lfo_bb.crt(x)).all() and (fc.matvec_bb(I, x) == lfo_bb.icrt(x)).all() and (fc.matvec_bb(I, g) == x).all()
            if count <= 65:
                rows += list(x) + list(g)
    hits, top = fc.icrt_group_classes(I, rows)
    nz = max(sum(1 for c in range(9) if I[i][9 * g + c]) for i in range(72) for g in range(8))
    print(f"icrt: largest group {top:.4f} 2^63, at most {nz} non-zero matrix entries per group")
    # the shipped inverse map has one non-zero entry per group (one per slot): a group is a single product, |T| <= H^2 = 0.11 2^63 -- the top of the column
    # and the pre-centring belong to denser maps; what remains is the second centring
    _report("icrt groups", hits, allowed=TOP if nz == 1 else ())
    assert top > 0.10 if nz == 1 else top > 0.5


# ---- the int8 paths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,l", fc.DOT_SHAPES_BB)
def test_int8_inner_product_operands(name, l):
    """the Y operand of k_dot_pack_y / k_bbdot_i8 in the decomposition of fc.dot_case_bb is row DOT_I0 of each matrix: with eq(r) the indicator of that row the
    oracle's u_s equal the big-integer inner products <z_k, row>, and the row's words carry a -128 and a 127 at every digit position, with carries"""
    from latticefold_amd.workload import make_workload
    wl, r = fc.dot_case_bb(name, l)
    assert wl.n >= 64 and (wl.n % 64 == 0) == (l == 63)
    ref = fc.Ref(BB)
    eq = ref.eq_table(fc.exts(r[:, :9]))
    assert [i for i, e in enumerate(eq) if any(e)] == [fc.DOT_I0] and eq[fc.DOT_I0] == ref.one
    inst = lfo_bb.Instance(wl)
    f = inst.witness_from_w_ccs(wl.w_ccs)
    cm = lfo_bb.ajtai_commit(inst.ajtai_matrix(), wl.kappa, wl.N, lfo_bb.crt(f))
    lc = _lcccs(wl, inst, cm, f, r)
    lcs, proof = inst.decomposition_prove(lfo_bb.Transcript(), inst.ajtai_matrix(), lc, f)
    t = wl.t
    assert proof.shape == (wl.K * (t + 9 + wl.l + 1 + wl.kappa), 72) and proof[:wl.K * t].any()
    y =np.concatenate([np.asarray(wl.val[j])[int(wl.rowptr[j][fc.DOT_I0]):int(wl.rowptr[j][fc.DOT_I0 + 1])] for j in range(t)])
    assert y.shape == (t * wl.n, 72)
    _report(f"int8 dot Y/{name}/l{l}", fc.count_classes_dig(y.reshape(-1)))
    run = max(len(s) for s in "".join("x" if int(v) == fc.canon(-0x3B808080) else " " for v in y[:, 0]).split())
    assert run >= 8
    # the X side of this entry point are the decomposed witness and public input: digits 0, +-1, i.e. the words 0, +-R, whose own base-256 digits are
    # (-2, 0, 0, 16) and (2, 0, 0, -16).  No X digit is -128, so a (-128) (-128) digit product cannot be formed through the decomposition prover; the largest
    # digit products it reaches are 16 x -128 and 16 x 127
    assert fc.digits_bb(fc.RB)[0] == [-2, 0, 0, 16] and fc.digits_bb(-fc.RB)[0] == [2, 0, 0, -16]


def _lcccs(wl, inst, cm, f, r):
    """an LCCCS (r, v, cm, u, x_w, h) at the given point: the oracle's linearization with r overwritten (the decomposition reads r, cm and x_w from it)"""
    cccs = np.concatenate([cm, wl.x_ccs])
    lc, _ = inst.linearize(lfo_bb.Transcript(), cccs, f)
    lc = lc.copy()
    lc[:wl.s] = r
    return lc


def test_int8_accumulator_guard_arithmetic():
    """launch_dot_batch_i8 refuses a shape whose waves would add 2048 or more steps of 64 digit products (each at most 2^14) into one int32: 2047 * 64 * 2^14 <
    2^31 <= 2048 * 64 * 2^14.  The guard's formula, restated from DotPlan::make (lf_dot_i8.cuh) with BabyBear's 12 chunks, flips between 12 * 2047 and
    12 * 2047 + 1 steps"""
    assert 2047 * 64 * 2**14 < 2**31 <= 2048 * 64 * 2**14
    edge = 12 * 2047 * 64
    assert fc.bbdot_guard(edge) == 0 and fc.bbdot_guard(edge - 63) == 0 and fc.bbdot_guard(edge + 1) == -1 and fc.bbdot_guard(64) == 0 and fc.bbdot_guard(4096) == 0
    with open(os.path.join(CSRC, "bb_dot_i8.hip")) as fh:
        src = fh.read()
    with open(os.path.join(CSRC, "lf_dot_i8.cuh")) as fh:
        plan = fh.read()
    assert "return steps_per_chunk < 2048;" in plan and "constexpr u32 BBDOT_CHUNKS = 12;" in src
    assert src.count("!p.make(X, n, BBDOT_CHUNKS)) return I8_ERR_SHAPE;") == 2     # both launchers refuse through the plan


def test_coef_eval_eq_words():
    """k_bbce_i8 cuts the eq table into digits: with r = (x, 0, .., 0) its non-zero entries are 1 - x and x, corner words for the chosen x = canon(w)"""
    from latticefold_amd.workload import make_workload
    wl = make_workload("B6")
    ref = fc.Ref(BB)
    vals = []
    for w in fc.CE_WORDS_BB:
        r = fc.ce_point(wl, w)
        eq = ref.eq_table(fc.exts(r[:, :9]))
        assert [i for i, e in enumerate(eq) if any(e)] == [0, 1] and eq[1] == (fc.canon(w),) * 9
        vals += list(eq[0]) + list(eq[1])
    _report("int8 coef eq", fc.count_classes_dig(vals))


# ---- the host program ------------------------------------------------------------------------------------------------------------------
def test_bb_field_selftest_program_under_sanitizers():
    """make bb-field-selftest: bb_field.cuh's host side against `%` over the word grid and the saturating pairs under -fsanitize=address,undefined (a stand-alone
    program: nothing is loaded into this interpreter)"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "bb-field-selftest"])
    r = subprocess.run([os.path.join(CSRC, "build", "bb_field_selftest")], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "selftest ok" in out and "runtime error" not in out and "Sanitizer" not in out and "MISMATCH" not in out
    grid = [ln for ln in out.splitlines() if ln.strip().startswith("grid:")]
    assert [int(v) for v in grid[0].split()[1:]] == fc.EDGE_BW          # the program's copy of the grid is this module's
    assert "largest column: 0.98877" in out


def test_the_three_copies_of_the_word_grid_agree():
    """EDGE_BW here, GRID in bb_field_selftest.cpp (also printed by the program, above) and selftest_bb::GRID in bb_capi.cpp (the device self-test's operands)"""
    for name in ("bb_field_selftest.cpp", "bb_capi.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            body = re.search(r"\bGRID\[\w+\] = \{([^}]*)\}", f.read()).group(1)
        vals = eval("[" + body.replace("/", "//") + "]", {"__builtins__": {}}, {"H": fc.HB, "R32": fc.RB})
        assert vals == fc.EDGE_BW, name
    assert fc.SELFTEST_PAIRS_BB == 9 * len(fc.EDGE_BW) ** 2 + 2 * len(fc.saturating_pairs())
