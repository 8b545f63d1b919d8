"""On-device relation checks of the LatticeFold+ slice (lfplus_r1cs_check / lfplus_linb_check; kernels lfp_check.hip): R_ComR1CS (r1cs.rs:21-60) and R_LinB
(lin.rs:29-40) on the resident (A, f).  Bit-exact integers, no tolerances.  Expected values never come from the code under test:
  A f and the LinB evaluations   the oracle's Decomp::decompose (lfp.decompose) with B = 2^62 on witnesses with |centred f| < 2^61: then F0 = f, so C0 = A f and v0
                                 holds the evaluations of f and M_j f at both points (F1 == 0 is asserted, so the trick cannot silently stop holding)
  the R1CS residual              a CSR product over lfp.ring_mul / lfp.addmod written here
  the real accumulator           lfp.PlusOracle.prove"""
import ctypes as C

import numpy as np
import pytest

import lfp
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
D, P = 16, plus.P
CM, R1CS, V, NORM = plus.REL_CM, plus.REL_R1CS, plus.REL_V, plus.REL_NORM
HALF = (P - 1) // 2


def centred_abs_max(f):
    f = np.asarray(f, dtype=np.uint64)
    return int(np.where(f <= np.uint64(HALF), f, np.uint64(P) - f).max())


def csr_rows(mat, f):
    """(M f) for a CSR matrix with ring coefficients: (n, 16) canonical words, through the oracle's ring product"""
    rowptr, col, val = (np.asarray(x) for x in mat)
    out = np.zeros((rowptr.size - 1, D), dtype=np.uint64)
    for r in np.nonzero(np.diff(rowptr.astype(np.int64)))[0]:
        acc = np.zeros(D, dtype=np.uint64)
        for k in range(int(rowptr[r]), int(rowptr[r + 1])):
            acc = lfp.addmod(acc, lfp.ring_mul(val[k], f[col[k]]))
        out[r] = acc
    return out


def host_first_bad(r1cs, f):
    """smallest row with ((M_A f) (M_B f) - M_C f) != 0, n when none"""
    ga, gb, gc = (csr_rows(m, f) for m in r1cs)
    for r in np.nonzero(ga.any(axis=1) | gc.any(axis=1))[0]:       # (a row with g_A = 0 and g_C = 0 holds)
        if (lfp.ring_mul(ga[r], gb[r]) != gc[r]).any():
            return int(r)
    return f.shape[0]


def host_mle(f, r):
    """mle(f)(r) for a point of ring CONSTANTS r (python ints), bit 0 of the row index <-> r[0]: 16 canonical words"""
    tab = [[int(x) for x in row] for row in f]
    for x in r:
        tab = [[(lo + x * (hi - lo)) % P for lo, hi in zip(tab[2 * j], tab[2 * j + 1])] for j in range(len(tab) // 2)]
    return np.array(tab[0], dtype=np.uint64)


def small_f(rng, n, bits=61):
    """n ring elements with |centred coefficient| < 2^bits, both signs"""
    mag = rng.integers(0, 1 << bits, size=(n, D), dtype=np.uint64)
    neg = rng.integers(0, 2, size=(n, D)).astype(bool) & (mag != 0)
    return np.where(neg, np.uint64(P) - mag, mag)


def const_points(rng, nvars):
    r = np.zeros((nvars, 2, D), dtype=np.uint64)
    r[:, :, 0] = rng.integers(0, P, size=(nvars, 2), dtype=np.uint64)
    return r


def linb_from_oracle(f, A, r, mats):
    """(cm, v) of the LinB instance (f, r) from the oracle's decompose with B = 2^62"""
    dec = lfp.decompose(f, A, 1 << 62, np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1]), mats)
    assert not dec["F1"].any() and (dec["F0"] == f).all(), "B = 2^62 no longer leaves F0 = f"
    return dec["C0"], dec["v0"]


def bump(a, idx):
    """a copy with one word changed (still canonical)"""
    b = np.array(a, copy=True)
    b[idx] = np.uint64((int(b[idx]) + 1) % P)
    return b


def square_system(n, ring=False, seed=0):
    """f_i f_i = f_i for every row i (identity matrices; holds for binary constants).  ring: M_A and M_C carry the same random ring coefficient per row
    ((c f_i) f_i = c f_i still holds), so the residual runs through the negacyclic coefficient path"""
    eye = plus.identity_csr(n)
    if not ring:
        return (eye, eye, eye)
    c = np.random.default_rng(seed).integers(0, P, size=(n, D), dtype=np.uint64)
    return ((eye[0], eye[1], c), eye, (eye[0], eye[1], c))


def binary_f(rng, n):
    f = np.zeros((n, D), dtype=np.uint64)
    f[:, 0] = rng.integers(0, 2, size=n)
    return f


# ---- case 1: satisfied instances pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,resident_mats", [("P15", False), ("P16", True)])
def test_satisfied_workload_instances_pass(name, resident_mats):
    wl = plus.make_plus_workload(name)
    A, r1cs, n = wl.ajtai_matrix(), wl.r1cs(), wl.n
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        if resident_mats:
            ctx.set_matrices(list(r1cs))
        for i, build in enumerate((plus.ComR1CS.new, plus.ComR1CS.new_resident)):
            z = wl.z(i)
            f = lfp.gadget_decompose(z, wl.B, wl.k)
            cr = build(ctx, r1cs, z, 1, wl.B, wl.k)
            assert (cr.cm_f == lfp.commit(A, f)).all()
            assert host_first_bad(r1cs, f) == n
            ok, failed, first_bad, absmax = cr.check_relation(ctx, resident=resident_mats)
            assert (ok, failed, first_bad) == (True, 0, n), (name, build.__name__)
            assert absmax == centred_abs_max(f)
            assert cr.check_relation(ctx, bound=absmax + 1, resident=resident_mats)[:2] == (True, 0)
            assert (ctx.get_witness() == f).all()
    finally:
        ctx.close()


# ---- case 2: first bad row ------------------------------------------------------------------------------------------------------------------------
def _gapped_system(n, ring):
    """rows [0, n/2) empty, row n/2 + i: f_(n/2+i) f_(n/2+i) = f_(n/2+i)"""
    h = n // 2
    rowptr = np.concatenate([np.zeros(h + 1, dtype=np.uint32), np.arange(1, h + 1, dtype=np.uint32)])
    col = np.arange(h, n, dtype=np.uint32)
    one = np.zeros((h, D), dtype=np.uint64)
    one[:, 0] = 1
    c = np.random.default_rng(4).integers(0, P, size=(h, D), dtype=np.uint64) if ring else one
    return ((rowptr, col, c), (rowptr, col, one), (rowptr, col, c))


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("case", ["row0", "last", "two", "gap"])
def test_first_bad_row(case, ring):
    n = 1 << 10
    rng = np.random.default_rng(11)
    A = lfp.splitmix(31, 0, n * D).reshape(1, n, D)
    r1cs = _gapped_system(n, ring) if case == "gap" else square_system(n, ring, seed=2)
    f = binary_f(rng, n)
    bad_rows = {"row0": [0], "last": [n - 1], "two": [700, 257], "gap": [n // 2 + 5]}[case]
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        ctx.set_witness(f)
        cm = lfp.commit(A, f)
        assert host_first_bad(r1cs, f) == n
        assert ctx.r1cs_check(cm, r1cs) == (True, 0, n, 1)
        # a wrong commitment with a satisfied system: CM only
        assert ctx.r1cs_check(bump(cm, (0, 3)), r1cs) == (False, CM, n, 1)
        for row in bad_rows:
            f[row, 0] = 2                                   # 2 * 2 != 2
        want = host_first_bad(r1cs, f)
        assert want == min(bad_rows)
        ctx.set_witness(f)
        cm = lfp.commit(A, f)                               # recomputed by the oracle: CM still holds
        assert ctx.r1cs_check(cm, r1cs) == (False, R1CS, want, 2)
        assert ctx.r1cs_check(None, r1cs)[:3] == (False, R1CS, want)
    finally:
        ctx.close()


# ---- case 3: LinB against the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("points", ["const", "ring"])
@pytest.mark.parametrize("nM", [0, 3])
@pytest.mark.parametrize("nvars", [10, 12])
def test_linb_against_the_oracle(nvars, nM, points, monkeypatch):
    monkeypatch.delenv("LFPLUS_LINB_TABLES", raising=False)
    n, kappa = 1 << nvars, 2
    rng = np.random.default_rng(100 * nvars + 10 * nM + (points == "ring"))
    A = lfp.splitmix(41, 0, kappa * n * D).reshape(kappa, n, D)
    mats = [tuple(np.array(x, copy=True) for x in m) for m in plus.r1cs_decomposed_square((plus.identity_csr(n // 2),) * 3, n, 8, 2)][:nM]
    f = small_f(rng, n)
    if points == "const":
        r = const_points(rng, nvars)
    else:
        r = rng.integers(0, P, size=(nvars, 2, D), dtype=np.uint64)
        if nM:
            mats[0][2][1, :] = rng.integers(0, P, size=D, dtype=np.uint64)      # a ring-valued coefficient as well
    cm, v = linb_from_oracle(f, A, r, mats)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        ctx.set_witness(f)
        amax = centred_abs_max(f)
        modes = (None, "1") if points == "const" else (None,)     # constant input: the one-pass path and (LFPLUS_LINB_TABLES) the table path must agree
        for mode in modes:
            if mode:
                monkeypatch.setenv("LFPLUS_LINB_TABLES", mode)
            assert ctx.linb_check(cm, r, v, mats) == (True, 0, amax), mode
            assert ctx.linb_check(bump(cm, (kappa - 1, 7)), r, v, mats) == (False, CM, amax), mode
            for q in range(1 + nM):
                for pt in range(2):
                    assert ctx.linb_check(cm, r, bump(v, (q, pt, (3 * q + pt) % D)), mats) == (False, V, amax), (mode, q, pt)
        monkeypatch.delenv("LFPLUS_LINB_TABLES", raising=False)
        if nM:                                                    # the same through resident matrices
            ctx.set_matrices(mats)
            assert ctx.linb_check(cm, r, v, plus.RESIDENT(nM)) == (True, 0, amax)
        assert (ctx.get_witness() == f).all()
    finally:
        ctx.close()


# ---- case 4: norm boundary and worst-case words -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", [False, True])
def test_norm_boundary_and_worst_case_words(tables, monkeypatch):
    if tables:
        monkeypatch.setenv("LFPLUS_LINB_TABLES", "1")
    else:
        monkeypatch.delenv("LFPLUS_LINB_TABLES", raising=False)
    nvars = 10
    n = 1 << nvars
    rng = np.random.default_rng(17)
    A = lfp.splitmix(43, 0, n * D).reshape(1, n, D)
    r = const_points(rng, nvars)
    pts = [[int(x) for x in r[:, pt, 0]] for pt in range(2)]
    # the python-int mle agrees with the oracle where the oracle can be asked (small f) ...
    fs = small_f(rng, n)
    _, vs = linb_from_oracle(fs, A, r, [])
    assert all((host_mle(fs, pts[pt]) == vs[0, pt]).all() for pt in range(2))
    # ... and gives the evaluations of a witness of worst-case words
    edge = np.array([0, 1, P - 1, HALF, HALF + 1], dtype=np.uint64)
    f = edge[rng.integers(0, edge.size, size=(n, D))]
    f[:5, 0], f[n - 5:, D - 1] = edge, edge
    v = np.stack([host_mle(f, pts[pt]) for pt in range(2)])[None]
    cm = lfp.commit(A, f)
    empty = (np.concatenate([np.zeros(1, dtype=np.uint32), np.ones(n, dtype=np.uint32)]), np.zeros(1, dtype=np.uint32), np.zeros((1, D), dtype=np.uint64))     # one zero coefficient: 0 * 0 = 0 holds for every f
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        for wit, amax in ((f, HALF), (np.where(f == np.uint64(HALF), np.uint64(HALF + 1), f), HALF), (np.where(f >= np.uint64(HALF), np.uint64(P - 1), f), 1)):
            ctx.set_witness(wit)
            if wit is not f:
                v, cm = np.stack([host_mle(wit, pts[pt]) for pt in range(2)])[None], lfp.commit(A, wit)
            assert ctx.linb_check(cm, r, v) == (True, 0, amax)                         # bound 0: the norm is not checked
            assert ctx.linb_check(cm, r, v, bound=amax) == (False, NORM, amax)         # absmax < bound is strict
            assert ctx.linb_check(cm, r, v, bound=amax + 1) == (True, 0, amax)
            assert ctx.r1cs_check(cm, (empty,) * 3) == (True, 0, n, amax)
            assert ctx.r1cs_check(cm, (empty,) * 3, bound=amax) == (False, NORM, n, amax)
            assert ctx.r1cs_check(cm, (empty,) * 3, bound=amax + 1) == (True, 0, n, amax)
    finally:
        ctx.close()


# ---- case 5: the decider on a real chain ----------------------------------------------------------------------------------------------------------
def _flat(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [v for y in x for v in _flat(y)]
    return [np.asarray(x)]


def test_decider_on_a_real_chain():
    wl = plus.make_plus_workload("P15")
    A, r1cs = wl.ajtai_matrix(), wl.r1cs()
    steps = ([wl.z(0), wl.z(1), wl.z(2)], [wl.z(3)])
    oracle = lfp.PlusOracle(A, list(r1cs), wl.kappa, 8, wl.k, wl.l, wl.B, lfp.Transcript())
    want_acc = []
    for zs in steps:
        oracle.prove([(lfp.gadget_decompose(z, wl.B, wl.k), r1cs) for z in zs])
        want_acc.append([np.array(a, copy=True) for a in oracle.acc])

    def run(device_acc, decide):
        prover = plus.PlusProver.init(A, list(r1cs), 1, wl.params(), plus.PoseidonTranscript(), 0)
        prover.device_acc = device_acc
        verdicts, proofs = [], []
        try:
            for s, zs in enumerate(steps):
                proof = prover.prove(prover.ingest(zs, r1cs))
                proofs.append(proof)
                if decide:
                    verdicts.append(prover.decide(proof))
                    bad = {**proof, "dproof": {**proof["dproof"], "v1": bump(proof["dproof"]["v1"], (1 + s, s, 5))}}
                    verdicts.append(prover.decide(bad))
                acc = prover.accumulator()
                assert all((acc[i] == want_acc[s][i]).all() for i in range(2)), "the accumulator differs from the oracle's"
            return proofs, verdicts, prover.transcript.get_challenge()
        finally:
            prover.close()
            plus.scratch_trim(0)

    for device_acc in (True, False):
        plain, _, ch0 = run(device_acc, False)
        proofs, verdicts, ch1 = run(device_acc, True)
        assert ch0 == ch1 == oracle.tr.clone().challenge()
        for a, b in zip(_flat(plain), _flat(proofs)):
            assert a.shape == b.shape and (a == b).all(), "a decide() between two proves changed the second proof"
        for s in range(2):
            good, tampered = verdicts[2 * s], verdicts[2 * s + 1]
            assert [x[:2] for x in good] == [(True, 0), (True, 0)], (device_acc, s, good)
            assert [x[:2] for x in tampered] == [(True, 0), (False, V)], (device_acc, s, tampered)
            assert [x[2] for x in good] == [centred_abs_max(want_acc[s][i]) for i in range(2)]


# ---- case 6: read-only ----------------------------------------------------------------------------------------------------------------------------
def test_checks_are_read_only_and_join_a_pending_from_f():
    n, kappa, k = 1 << 15, 1, 2
    dp = plus.DecompParameters.for_frog(k)
    A = lfp.splitmix(1, 0, kappa * n * D).reshape(kappa, n, D)
    vv = (lfp.splitmix(2, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    f = np.where(vv < 0, np.uint64(P) - (-vv).astype(np.uint64), vv.astype(np.uint64)).reshape(n, D)
    want = lfp.rg_from_f(f, A, dp.b, dp.k, dp.l)
    r1cs = square_system(n)
    r = const_points(np.random.default_rng(5), 15)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        ctx.set_witness(f)
        before = ctx.get_witness()
        ctx.rg_from_f_async(dp)                             # in flight on the second stream while the checks are issued
        res1 = ctx.r1cs_check(want["cm_f"], r1cs)
        res2 = ctx.linb_check(want["cm_f"], r, np.zeros((1, 2, D), dtype=np.uint64))
        assert res1[:2] == (False, R1CS) and res2[:2] == (False, V) and res1[3] == res2[2] == 31
        assert (ctx.get_witness() == before).all() and (before == f).all()
        L = plus._lib()
        ctx._chk(L.lfplus_rg_from_f(ctx.h, dp.b, dp.k, dp.l))            # collects the pass issued before the checks
        Df, com = np.zeros((k, n, D), dtype=np.int8), np.zeros((k, kappa, D, D), dtype=np.uint64)
        tau, mt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int8)
        c3 = [np.zeros((kappa, D), dtype=np.uint64) for _ in range(3)]
        ctx._chk(L.lfplus_rg_read(ctx.h, Df.ctypes.data_as(plus.i8p), com.ctypes.data_as(plus.u64p), tau.ctypes.data_as(plus.u64p), mt.ctypes.data_as(plus.i8p),
                                  *[x.ctypes.data_as(plus.u64p) for x in c3]))
        assert (Df == want["Df"]).all() and (com == want["comMf"]).all() and (tau == want["tau"]).all()
        assert (c3[0] == want["cm_f"]).all() and (c3[1] == want["C_Mf"]).all() and (c3[2] == want["cm_mtau"]).all()
        assert ctx.r1cs_check(want["cm_f"], r1cs) == res1 and (ctx.get_witness() == f).all()
    finally:
        ctx.close()


# ---- case 7: error codes --------------------------------------------------------------------------------------------------------------------------
def _e_arg(fn):
    with pytest.raises(plus.LfPlusError) as e:
        fn()
    assert e.value.code == plus.E_ARG


def test_error_codes_leave_the_context_usable():
    nvars = 10
    n = 1 << nvars
    rng = np.random.default_rng(23)
    A = lfp.splitmix(47, 0, n * D).reshape(1, n, D)
    f = binary_f(rng, n)
    r1cs = square_system(n)
    r = const_points(rng, nvars)
    cm, v = linb_from_oracle(f, A, r, [])
    ctx = plus.PlusContext(0)
    try:
        _e_arg(lambda: ctx.r1cs_check(None, r1cs))                                   # no commitment matrix, no witness
        ctx.kappa, ctx.n = 1, n
        _e_arg(lambda: ctx.linb_check(None, r, v))
        ctx.set_matrix(A)
        _e_arg(lambda: ctx.r1cs_check(cm, r1cs))                                     # no witness
        _e_arg(lambda: ctx.linb_check(cm, r, v))
        ctx.set_witness(f)
        good = lambda: ctx.r1cs_check(cm, r1cs) == (True, 0, n, 1) and ctx.linb_check(cm, r, v) == (True, 0, 1)
        assert good()
        _e_arg(lambda: ctx.r1cs_check(cm))                                           # no resident matrices
        ctx.set_matrices(list(r1cs[:2]))
        _e_arg(lambda: ctx.r1cs_check(cm))                                           # two resident matrices: an R1CS has three
        _e_arg(lambda: ctx.linb_check(cm, r, np.zeros((4, 2, D), dtype=np.uint64), plus.RESIDENT(3)))
        assert good()
        ctx.set_matrices(list(r1cs))
        assert ctx.r1cs_check(cm) == (True, 0, n, 1)
        def poisoned(a, idx, word):
            b = np.array(a, copy=True)
            b[idx] = np.uint64(word)
            return b
        for bad_cm, bad_r, bad_v in ((poisoned(cm, (0, 2), P), r, v), (cm, poisoned(r, (3, 1, 0), P + 1), v), (cm, r, poisoned(v, (0, 1, 15), 2**64 - 1))):
            _e_arg(lambda: ctx.linb_check(bad_cm, bad_r, bad_v))
            assert good()
        _e_arg(lambda: ctx.r1cs_check(poisoned(cm, (0, 9), P), r1cs))
        bad_csr = (r1cs[0], (r1cs[1][0], np.full(n, n, dtype=np.uint32), r1cs[1][2]), r1cs[2])       # column index out of range
        _e_arg(lambda: ctx.r1cs_check(cm, bad_csr))
        _e_arg(lambda: ctx.linb_check(cm, r, np.zeros((2, 2, D), dtype=np.uint64), [bad_csr[1]]))
        assert good()
        # a NULL `failed`
        L = plus._lib()
        keep, rp, cp, vp = plus._csr_args(r1cs)
        fb, am = C.c_uint64(), C.c_uint64()
        assert L.lfplus_r1cs_check(ctx.h, None, rp, cp, vp, 0, None, C.byref(fb), C.byref(am)) == plus.E_ARG
        ra, rb = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        assert L.lfplus_linb_check(ctx.h, None, ra.ctypes.data_as(plus.u64p), rb.ctypes.data_as(plus.u64p), 0, None, None, None, v.ctypes.data_as(plus.u64p), 0, None,
                                   C.byref(am)) == plus.E_ARG
        assert good()
    finally:
        ctx.close()
    # a sharded context (the timing model of rank 0 of 2): refused like lfplus_witness_from_z
    sh = plus.PlusContext(0)
    try:
        sh.set_sharding_model(0, 2)
        sh.set_matrix(A[:, :n // 2])
        sh.set_witness(f)
        _e_arg(lambda: sh.r1cs_check(cm, r1cs))
        _e_arg(lambda: sh.linb_check(cm, r, v))
        assert (sh.get_witness() == f).all()
    finally:
        sh.close()
