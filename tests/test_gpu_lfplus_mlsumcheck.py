"""The LatticeFold+ generic sumcheck on the device (lfplus_mlsumcheck_*, include/lfplus.h) against the Python reference of tests/lfplus_mlsumcheck_ref.py and
the oracle's ComR1CS::linearize (oracle/lfp_protocol.c through tests/lfp.py): round by round through the split form and in one call through prove, host and
device tables, the refusals in their stated order, the state machine, and the independence from everything else a context holds.  Bit-exact: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import lfp
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
P, D = plus.P, plus.D
E_ARG = plus.E_ARG
SENT = 0x5A5A5A5A5A5A5A5A
u64p = plus.u64p
u32p = C.POINTER(C.c_uint32)


def L():
    return plus._lib()


def err(ctx):
    return L().lfplus_last_error(ctx.h).decode()


def hp(a):
    return a.ctypes.data_as(u64p)


def dev_view(a):
    """the words of `a` as a view at a non-zero, 16-byte aligned offset of a larger device allocation -> (view, the whole allocation)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    whole = torch.full((a.size + 6,), SENT, dtype=torch.int64, device="cuda")
    view = whole[2:2 + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a.view(np.int64).copy()))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != whole.data_ptr()
    return view, whole


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = plus.PlusContext(0)      # BARE: no matrix, no witness
    yield c
    c.close()


def run_split(ctx, tables, terms, degree, point):
    """the split form on the reference's challenges -> (msgs, final)"""
    sc = plus.MLSumcheck(ctx, tables, plus.VPoly(terms, degree))
    msgs = [sc.prove_round()]
    for r in point[:-1]:
        msgs.append(sc.prove_round(int(r)))
    fin = sc.final(int(point[-1]))
    sc.end()
    return np.stack(msgs), fin


def check_case(ctx, shape, nvars):
    tables, terms, degree, msgs, point, final = ref.case(shape, nvars)
    got_m, got_f = run_split(ctx, tables, terms, degree, point)
    assert np.array_equal(got_m, msgs), "split form: round messages"
    assert np.array_equal(got_f, final), "split form: final"
    m2, p2, f2 = plus.mlsumcheck_prove(ctx, plus.PoseidonTranscript(), tables, plus.VPoly(terms, degree))
    assert np.array_equal(m2, msgs) and np.array_equal(p2, point) and np.array_equal(f2, final), "prove"
    # the host verifier on the device proof: accepted, expected = g(final), the transcripts agree
    tp, tv = plus.PoseidonTranscript(), plus.PoseidonTranscript()
    m3, _, f3 = plus.mlsumcheck_prove(ctx, tp, tables, plus.VPoly(terms, degree))
    ok, pt, expected = plus.mlsumcheck_verify(tv, nvars, degree, plus.mlsumcheck_extract_sum(m3), m3)
    assert ok and np.array_equal(pt, point) and np.array_equal(expected, ref.g_at(f3, terms))
    assert tp.get_challenge() == tv.get_challenge()


# nvars 1: a single round, final follows round 1; 2; 4: 8 pairs, half a workgroup; 5: exactly one; 6: two; 9
@pytest.mark.parametrize("nvars", [1, 2, 4, 5, 6, 9])
@pytest.mark.parametrize("shape", ["a", "b", "e", "f-max", "f-mix"])
def test_shapes_against_the_reference(ctx, shape, nvars):
    check_case(ctx, shape, nvars)


@pytest.mark.parametrize("shape,nvars", [("c", 1), ("c", 3), ("c", 4), ("d", 2), ("d", 5)])
def test_envelope_and_claimed_degree(ctx, shape, nvars):
    """c: 16 tables, 16 terms, an 8-factor term, degree 8, 64 factors (small: the reference is slow there); d: claimed degree 5 over two factors at most"""
    check_case(ctx, shape, nvars)


@pytest.mark.parametrize("cap", [3, 1])
def test_the_block_cap_forces_the_grid_stride_loop(ctx, monkeypatch, cap):
    """nvars 9: 256 pairs = 16 groups of 16 in round 1; three workgroups take 6 / 5 / 5 of them (an uneven remainder), one takes all 16"""
    monkeypatch.setenv("LFPLUS_MLS_BLOCKS", str(cap))
    check_case(ctx, "b", 9)
    check_case(ctx, "e", 6)


# ---- the oracle pin at size ----------------------------------------------------------------------------------------------------------------------------------------
def test_r1cs_shape_at_nvars_12_is_the_oracle_linearization(ctx):
    nvars = 12
    n = 1 << nvars
    f = ref.rand_ring(0x91, (n, D))
    r1cs = [ref.rand_csr(0x92 + q, n, 2) for q in range(3)]
    seed = ref.rand_ring(0x95, (3, D))
    tr_o, tr_p, tr_g = lfp.Transcript(), plus.PoseidonTranscript(), plus.PoseidonTranscript()
    for t in (tr_o, tr_p, tr_g):
        t.absorb(seed)
    want = lfp.r1cs_linearize(tr_o, nvars, f, r1cs)
    r = [tr_g.get_challenge() for _ in range(nvars)]                        # from a transcript in the same state, as ComR1CS::linearize draws it
    tables = ref.r1cs_tables(r, f, r1cs)
    msgs, point, fin = plus.mlsumcheck_prove(ctx, tr_g, tables, plus.VPoly(ref.R1CS_TERMS, 3))
    assert np.array_equal(msgs, want["msgs"]) and np.array_equal(point, want["r"]) and np.array_equal(fin[1:], want["evals"][1:])
    # and the product's own ComR1CS::linearize, on a second context
    c2 = plus.PlusContext(0)
    try:
        c2.set_matrix(ref.rand_ring(0x96, (1, n, D)))
        linb, proof = plus.ComR1CS(tuple(r1cs), None, f, None).linearize(c2, tr_p)
    finally:
        c2.close()
    assert np.array_equal(msgs, proof["msgs"]) and np.array_equal(point, proof["r"]) and np.array_equal(fin[1:], proof["evals"][1:])


# ---- host and device tables ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nvars", [("b", 1), ("a", 2), ("b", 6), ("e", 9)])
def test_device_tables_give_the_host_words_and_are_not_written(ctx, shape, nvars):
    tables, terms, degree, msgs, point, final = ref.case(shape, nvars)
    view, whole = dev_view(tables)
    before = host(whole).copy()
    got_m, got_f = run_split(ctx, view, terms, degree, point)
    assert np.array_equal(got_m, msgs) and np.array_equal(got_f, final)
    m2, p2, f2 = plus.mlsumcheck_prove(ctx, plus.PoseidonTranscript(), view, plus.VPoly(terms, degree))
    assert np.array_equal(m2, msgs) and np.array_equal(p2, point) and np.array_equal(f2, final)
    assert np.array_equal(host(whole), before), "the caller's tensor (and its surroundings) is unchanged"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def raw_desc(nvars, T, q, degree, off, idx, coef):
    off, idx, coef = np.asarray(off, dtype=np.uint32), np.asarray(list(idx) + [0], dtype=np.uint32), np.ascontiguousarray(coef, dtype=np.uint64)
    d = plus.VPolyDesc(nvars, T, q, degree, off.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), hp(coef))
    d._keep = (off, idx, coef)
    return d


def in_progress(ctx):
    """a sumcheck with round 1 answered -> a function that answers round 2 and final and compares them with the reference"""
    tables, terms, degree, msgs, point, final = ref.case("b", 4)
    sc = plus.MLSumcheck(ctx, tables, plus.VPoly(terms, degree))
    assert np.array_equal(sc.prove_round(), msgs[0])

    def still_there():
        assert np.array_equal(sc.prove_round(int(point[0])), msgs[1])
        for i in (2, 3):
            assert np.array_equal(sc.prove_round(int(point[i - 1])), msgs[i])
        assert np.array_equal(sc.final(int(point[3])), final)
        sc.end()
    return still_there


def test_refusals_in_their_stated_order(ctx):
    tables, terms, degree, msgs, point, final = ref.case("b", 2)          # 4 tables, 5 terms, degree 3
    T, nv = 4, 2
    off, idx = [0, 2, 4, 6, 9, 10], [0, 1, 1, 2, 3, 3, 2, 2, 2, 0]
    coef = np.stack([np.asarray(c, dtype=np.uint64) for c, _ in terms])
    good = raw_desc(nv, T, 5, 3, off, idx, coef)
    t = np.ascontiguousarray(tables)
    bad_idx = list(idx); bad_idx[3] = 4
    bad_off = list(off); bad_off[2] = 2
    bad_coef = coef.copy(); bad_coef[4, 15] = P
    bad_tab = t.copy(); bad_tab[3, 3, 15] = P
    sharded = plus.PlusContext(0)
    sharded.set_sharding_model(0, 2)
    still_there = in_progress(ctx)
    msgs_o, point_o, fin_o = (np.full(s, SENT, dtype=np.uint64) for s in ((nv, 4, D), (nv,), (T, D)))
    fresh = plus.PoseidonTranscript().get_challenge()
    tr = plus.PoseidonTranscript()
    try:
        # (what is wrong, descriptor, tables, context, what the message names)
        cases = [
            ("null + index", raw_desc(nv, T, 5, 3, off, bad_idx, coef), None, ctx, "null"),
            ("index + offsets", raw_desc(nv, T, 5, 3, bad_off, bad_idx, coef), t, ctx, "table index"),
            ("offsets + coefficient", raw_desc(nv, T, 5, 3, bad_off, idx, bad_coef), t, ctx, "term_off"),
            ("coefficient + envelope", raw_desc(nv, T, 5, 9, off, idx, bad_coef), t, ctx, "coefficient"),
            ("envelope (degree below the widest term) + sharded", raw_desc(nv, T, 5, 2, off, idx, coef), t, sharded, "factors"),
            ("envelope: nvars 0", raw_desc(0, T, 5, 3, off, idx, coef), t, ctx, "envelope"),
            ("envelope: nvars 29", raw_desc(29, T, 5, 3, off, idx, coef), t, ctx, "envelope"),
            ("envelope: 17 tables", raw_desc(nv, 17, 5, 3, off, idx, coef), t, ctx, "envelope"),
            ("envelope: no term", raw_desc(nv, T, 0, 3, off, idx, coef), t, ctx, "envelope"),
            ("sharded + table word", good, bad_tab, sharded, "sharded"),
            ("table word", good, bad_tab, ctx, "non-canonical table word"),
        ]
        for name, d, tab, c, word in cases:
            p = hp(tab) if tab is not None else None
            assert L().lfplus_mlsumcheck_begin(c.h, C.byref(d), p) == E_ARG and word in err(c), (name, err(c))
            assert L().lfplus_mlsumcheck_prove(c.h, tr.h, C.byref(d), p, hp(msgs_o), hp(point_o), hp(fin_o)) == E_ARG and word in err(c), (name, err(c))
        assert L().lfplus_mlsumcheck_begin(ctx.h, None, hp(t)) == E_ARG and "null" in err(ctx)
        assert L().lfplus_mlsumcheck_prove(ctx.h, None, C.byref(good), hp(t), hp(msgs_o), hp(point_o), hp(fin_o)) == E_ARG and "null" in err(ctx)
        assert L().lfplus_mlsumcheck_prove(ctx.h, tr.h, C.byref(good), hp(t), None, hp(point_o), hp(fin_o)) == E_ARG and "null" in err(ctx)
        assert L().lfplus_mlsumcheck_prove(ctx.h, tr.h, C.byref(good), hp(t), hp(msgs_o), None, hp(fin_o)) == E_ARG and "null" in err(ctx)
        assert all((a == SENT).all() for a in (msgs_o, point_o, fin_o)), "no output is written"
        assert tr.clone().get_challenge() == fresh, "a refused prove leaves the transcript alone"
        still_there()                                                      # the sumcheck in progress was left as it was, and the context is usable
        assert L().lfplus_mlsumcheck_prove(ctx.h, plus.PoseidonTranscript().h, C.byref(good), hp(t), hp(msgs_o), hp(point_o), None) == 0      # final_out may be NULL
        assert np.array_equal(msgs_o, msgs) and np.array_equal(point_o, point)
    finally:
        sharded.close()


def test_the_state_machine(ctx):
    tables, terms, degree, msgs, point, final = ref.case("a", 2)
    lib = L()
    o, r = np.zeros((degree + 1, D), dtype=np.uint64), C.c_uint64(int(point[0]))
    fo = np.zeros((tables.shape[0], D), dtype=np.uint64)
    lib.lfplus_mlsumcheck_end(ctx.h)
    assert lib.lfplus_mlsumcheck_round(ctx.h, None, hp(o)) == E_ARG and "no sumcheck" in err(ctx)                       # round before begin
    assert lib.lfplus_mlsumcheck_final(ctx.h, C.byref(r), hp(fo)) == E_ARG and "no sumcheck" in err(ctx)
    sc = plus.MLSumcheck(ctx, tables, plus.VPoly(terms, degree))
    assert lib.lfplus_mlsumcheck_round(ctx.h, C.byref(r), hp(o)) == E_ARG and "round 1" in err(ctx)                     # a challenge in round 1
    assert lib.lfplus_mlsumcheck_final(ctx.h, C.byref(r), hp(fo)) == E_ARG and "still" in err(ctx)                      # final before the last round
    assert np.array_equal(sc.prove_round(), msgs[0])
    assert lib.lfplus_mlsumcheck_round(ctx.h, None, hp(o)) == E_ARG and "NULL" in err(ctx)                              # no challenge in a later round
    big = C.c_uint64(P)
    assert lib.lfplus_mlsumcheck_round(ctx.h, C.byref(big), hp(o)) == E_ARG and "non-canonical" in err(ctx)
    assert lib.lfplus_mlsumcheck_final(ctx.h, C.byref(r), hp(fo)) == E_ARG and "still" in err(ctx)
    assert np.array_equal(sc.prove_round(int(point[0])), msgs[1])                                                       # (none of the refusals moved the state)
    r1 = C.c_uint64(int(point[1]))
    assert lib.lfplus_mlsumcheck_round(ctx.h, C.byref(r1), hp(o)) == E_ARG and "answered" in err(ctx)                   # more than nvars rounds
    assert np.array_equal(sc.final(int(point[1])), final)
    # begin while a sumcheck is active replaces it
    t2, terms2, degree2, msgs2, point2, final2 = ref.case("b", 1)
    sc2 = plus.MLSumcheck(ctx, t2, plus.VPoly(terms2, degree2))
    assert np.array_equal(sc2.prove_round(), msgs2[0]) and np.array_equal(sc2.final(int(point2[0])), final2)
    sc2.end()
    assert lib.lfplus_mlsumcheck_round(ctx.h, None, hp(o)) == E_ARG and lib.lfplus_mlsumcheck_end(ctx.h) == 0


def test_device_table_refusals(ctx):
    tables, terms, degree, msgs, point, final = ref.case("b", 4)
    T, n = tables.shape[0], tables.shape[1]
    d = plus.VPoly(terms, degree).desc(4, T)
    words = T * n * D
    torch.cuda.empty_cache()
    big = torch.zeros((32 << 20) // 8, dtype=torch.int64, device="cuda")      # an allocation of its own (requested from an empty cache)
    pinned = torch.zeros((T * n, D), dtype=torch.int64).pin_memory()
    good, whole = dev_view(tables)
    torch.cuda.synchronize()
    bad = [("pinned host memory", pinned.data_ptr()), ("pageable host memory", np.ascontiguousarray(tables).ctypes.data), ("dev + 8", good.data_ptr() + 8),
           ("off the end", big.data_ptr() + (32 << 20) - 128), ("null", None)]
    still_there = in_progress(ctx)
    msgs_o, point_o, fin_o = (np.full(s, SENT, dtype=np.uint64) for s in ((4, degree + 1, D), (4,), (T, D)))
    tr = plus.PoseidonTranscript()
    fresh = plus.PoseidonTranscript().get_challenge()
    for name, addr in bad:
        p = C.c_void_p(addr)
        assert L().lfplus_mlsumcheck_begin_device(ctx.h, C.byref(d), p) == E_ARG and err(ctx), name
        assert L().lfplus_mlsumcheck_prove_device(ctx.h, tr.h, C.byref(d), p, hp(msgs_o), hp(point_o), hp(fin_o)) == E_ARG and err(ctx), name
    assert all((a == SENT).all() for a in (msgs_o, point_o, fin_o)) and tr.clone().get_challenge() == fresh
    still_there()
    # a device word >= p: found by the kernel that reads the tables; no sumcheck is left
    for entry in (plus.MLSumcheck, None):
        still = in_progress(ctx)
        t = np.ascontiguousarray(tables).copy()
        t[T - 1, n - 1, D - 1] = P
        view, w2 = dev_view(t)
        ctx.wait_stream()
        if entry is None:
            rc = L().lfplus_mlsumcheck_prove_device(ctx.h, tr.h, C.byref(d), C.c_void_p(view.data_ptr()), hp(msgs_o), hp(point_o), hp(fin_o))
        else:
            rc = L().lfplus_mlsumcheck_begin_device(ctx.h, C.byref(d), C.c_void_p(view.data_ptr()))
        assert rc == E_ARG and "non-canonical" in err(ctx)
        o = np.zeros((degree + 1, D), dtype=np.uint64)
        r = C.c_uint64(int(point[0]))
        assert L().lfplus_mlsumcheck_round(ctx.h, C.byref(r), hp(o)) == E_ARG and "no sumcheck" in err(ctx)
        del still
    assert all((a == SENT).all() for a in (msgs_o, point_o, fin_o)) and tr.clone().get_challenge() == fresh
    check_case(ctx, "b", 2)                                                  # the context stays usable


# ---- independence ------------------------------------------------------------------------------------------------------------------------------------------------
def _rg_read(c, k, kappa, n):
    Df, com = np.zeros((k, n, D), dtype=np.int8), np.zeros((k, kappa, D, D), dtype=np.uint64)
    tau, mt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int8)
    cs = [np.zeros((kappa, D), dtype=np.uint64) for _ in range(3)]
    c._chk(L().lfplus_rg_read(c.h, Df.ctypes.data_as(plus.i8p), hp(com), hp(tau), mt.ctypes.data_as(plus.i8p), *[hp(x) for x in cs]))
    return [Df, com, tau, mt] + cs


@pytest.mark.parametrize("pending", [False, True])
def test_a_loaded_context_is_not_disturbed(pending):
    n, kappa, k = 1 << 15, 1, 2                                               # (from_f needs n > kappa k d l d)
    dp = plus.DecompParameters.for_frog(k)
    A = lfp.splitmix(1, 0, kappa * n * D).reshape(kappa, n, D) % np.uint64(P)
    v = (lfp.splitmix(2, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    f = np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)
    r1cs = [ref.rand_csr(0x55 + q, n, 1) for q in range(3)]
    c = plus.PlusContext(0)
    try:
        c.set_matrix(A)
        c.set_matrices(r1cs)
        c.set_witness(f)
        c._chk(L().lfplus_rg_from_f(c.h, dp.b, dp.k, dp.l))
        want = _rg_read(c, k, kappa, n)
        c._chk((L().lfplus_rg_from_f_async if pending else L().lfplus_rg_from_f)(c.h, dp.b, dp.k, dp.l))
        check_case(c, "b", 6)                                                # a generic sumcheck between from_f and the read
        check_case(c, "e", 2)
        if pending:
            c._chk(L().lfplus_rg_from_f(c.h, dp.b, dp.k, dp.l))            # collects the pass
        got = _rg_read(c, k, kappa, n)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.array_equal(c.get_witness(), f)
        # the resident matrices still linearize as the oracle does
        tr_o, tr_p = lfp.Transcript(), plus.PoseidonTranscript()
        linb, proof = plus.ComR1CS(tuple(r1cs), None, None, None, 1, c).linearize(c, tr_p, resident=True)
        assert np.array_equal(proof["msgs"], lfp.r1cs_linearize(tr_o, 15, f, r1cs)["msgs"])
    finally:
        c.close()


def test_interleaved_with_a_linearization_on_a_second_context(ctx):
    nvars = 6
    n = 1 << nvars
    tables, terms, degree, msgs, point, final = ref.case("a", nvars)
    f = ref.rand_ring(0x61, (n, D))
    r1cs = [ref.rand_csr(0x62 + q, n, 2) for q in range(3)]
    want = lfp.r1cs_linearize(lfp.Transcript(), nvars, f, r1cs)
    c2 = plus.PlusContext(0)
    try:
        c2.set_matrix(ref.rand_ring(0x65, (1, n, D)))
        sc = plus.MLSumcheck(ctx, tables, plus.VPoly(terms, degree))
        for i in range(nvars):
            assert np.array_equal(sc.prove_round(None if i == 0 else int(point[i - 1])), msgs[i])
            linb, proof = plus.ComR1CS(tuple(r1cs), None, f, None).linearize(c2, plus.PoseidonTranscript())
            assert np.array_equal(proof["msgs"], want["msgs"]) and np.array_equal(proof["evals"], want["evals"])
        assert np.array_equal(sc.final(int(point[-1])), final)
        sc.end()
    finally:
        c2.close()
