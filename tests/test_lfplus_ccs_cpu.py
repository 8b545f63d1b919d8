"""Committed CCS instances without a GPU: the three entry points in header, library, Python mirror and generated binding; lfplus_ccs_verify (host only) on the
oracle's R1CS proofs and on proofs of the Python reference (tests/lfplus_ccs_ref.py) for general shapes; every refusal of the envelope, in the order
include/lfplus.h states; the answers of the device entry points when there is no device or no context."""
import ctypes as C
import os

import numpy as np
import pytest

import lfp
import lfplus_ccs_ref as cref
import lfplus_mlsumcheck_ref as ref
from latticefold_amd import plus

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMBOLS = ["lfplus_ccs_linearize", "lfplus_ccs_verify", "lfplus_ccs_check"]
P, D = plus.P, plus.D
u64p = plus.u64p
u32p = C.POINTER(C.c_uint32)


def _shape(sh):
    return plus.CCSShape(*sh)


def test_the_three_symbols_through_every_layer():
    names = plus.exported_symbols()
    lib = plus._lib()
    for s in SYMBOLS:
        assert s in names, f"include/lfplus.h does not declare {s}"
        assert hasattr(lib, s), f"liblfhip.so does not export {s}"
        assert getattr(lib, s).argtypes is not None, f"{s} has no argtypes in plus.py"
    sys_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    assert all(f"pub fn {s}(" in sys_rs for s in SYMBOLS) and "pub struct lfplus_ccs" in sys_rs and "pub const LFPLUS_REL_CCS: c_int = 2;" in sys_rs
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "plus.rs")).read()
    assert all(f"sys::{s}(" in safe for s in SYMBOLS)
    assert all(hasattr(plus, n) for n in ("CCSShape", "ComCCS", "ccs_verify")) and plus.REL_CCS == plus.REL_R1CS == 2
    assert "LFPLUS_CCS_BLOCKS" in open(os.path.join(ROOT, "SWITCHES.md")).read()


def test_shape_descriptor():
    g = ref.rand_ring(9, (D,))
    sh = plus.CCSShape(3, [[0, 1, 1], [2], [0]], [g, -1, 5])
    assert (sh.t, sh.q, sh.degree) == (3, 3, 3)
    d = sh.desc()
    assert (d.t, d.q) == (3, 3) and [d.S_off[i] for i in range(4)] == [0, 3, 4, 5] and [d.S_idx[i] for i in range(5)] == [0, 1, 1, 2, 0]
    c = np.ctypeslib.as_array(d.c, shape=(3, D))
    assert np.array_equal(c[0], g) and c[1, 0] == P - 1 and not c[1, 1:].any() and c[2, 0] == 5 and not c[2, 1:].any()
    r = plus.CCSShape.r1cs()
    assert (r.t, r.multisets, r.degree) == (3, [[0, 1], [2]], 2) and r.coeffs[0, 0] == 1 and r.coeffs[1, 0] == P - 1
    with pytest.raises(plus.LfPlusError):
        plus.CCSShape(2, [[0], [1]], [1])


@pytest.mark.parametrize("nvars", [3, 4])
def test_verify_r1cs_shape_on_the_oracle_proofs(nvars):
    """the oracle's ComR1CS proofs: accepted, with the ro of lfplus_r1cs_verify and the transcript left in the same state"""
    f, r1cs = cref.satisfied_r1cs(1 << nvars, 0x81 + nvars)
    tr_o = lfp.Transcript()
    tr_o.absorb(ref.rand_ring(0x83, (2, D)))
    want = lfp.r1cs_linearize(tr_o, nvars, f, r1cs)
    t_ccs, t_r1cs = plus.PoseidonTranscript(), plus.PoseidonTranscript()
    for t in (t_ccs, t_r1cs):
        t.absorb(ref.rand_ring(0x83, (2, D)))
    ok, st, ro = plus.ccs_verify(t_ccs, plus.CCSShape.r1cs(), want)
    ok2, st2, ro2 = plus.r1cs_verify(t_r1cs, want)
    assert ok and st == 0 and ok2 and st2 == 0
    assert np.array_equal(ro, ro2) and np.array_equal(ro, want["r"])
    nxt = t_ccs.get_challenge()
    assert nxt == t_r1cs.get_challenge() == tr_o.challenge()
    # and the rejections of the R1CS verifier, stage for stage (an evaluation beyond the first two of the LAST round moves only the expected evaluation: stage 2)
    for key, idx, stage in (("msgs", (nvars - 1, 1, 3), 1), ("msgs", (0, 3, 3), 1), ("msgs", (nvars - 1, 2, 3), 2), ("evals", (2, 7), 2), ("evals", (0, 0), 0)):
        bad = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in want.items()}
        bad[key][idx] ^= np.uint64(1)
        ta, tb = plus.PoseidonTranscript(), plus.PoseidonTranscript()
        for t in (ta, tb):
            t.absorb(ref.rand_ring(0x83, (2, D)))
        a, b = plus.ccs_verify(ta, plus.CCSShape.r1cs(), bad), plus.r1cs_verify(tb, bad)
        assert (a[0], a[1]) == (b[0], b[1]) == (stage == 0, stage)      # (v = evals[0] is not part of the identity: the LinB check is what binds it)


def _seeded():
    t = plus.PoseidonTranscript()
    t.absorb(ref.rand_ring(0x5EED, (2, D)))
    return t


@pytest.mark.parametrize("name,nvars", [("a", 1), ("b", 3), ("c", 5), ("d", 3), ("e", 1)])
def test_verify_accepts_and_rejects_by_stage(name, nvars):
    """proofs of the Python reference for satisfied instances of the general shapes (_vanishing_case): accepted, with the reference's ro and transcript state.
    A changed word of a message is rejected at stage 1 -- except an evaluation beyond the first two of the LAST round, which moves only the expected evaluation
    and is caught by the final identity (stage 2), exactly as in lfplus_r1cs_verify.  A changed word of evals[1:] is rejected at stage 2 whenever the identity
    depends on that evaluation (computed here with Python integers)"""
    sh, f, mats, proof = _vanishing_case(name, nvars)
    d = cref.degree_of(sh)
    ok, st, ro = plus.ccs_verify(_seeded(), _shape(sh), proof)
    assert ok and st == 0 and np.array_equal(ro, proof["r"])
    tr, tr_o = _seeded(), lfp.Transcript()
    tr_o.absorb(ref.rand_ring(0x5EED, (2, D)))
    plus.ccs_verify(tr, _shape(sh), proof)
    cref.replay(tr_o, sh, proof)
    assert tr.get_challenge() == tr_o.challenge(), "the transcript has advanced as the reference's schedule does"
    for rnd in sorted({0, nvars - 1}):
        for x in sorted({0, 1, d + 1}):
            bad = dict(proof, msgs=proof["msgs"].copy())
            bad["msgs"][rnd, x, 5] ^= np.uint64(1)
            ok, st, _ = plus.ccs_verify(_seeded(), _shape(sh), bad)
            if x >= 2 and rnd == nvars - 1:      # (an evaluation beyond the first two of the LAST round changes only the expected evaluation: the final identity fails)
                assert not ok and st == 2
            else:
                assert not ok and st == 1
    g = lambda ev: ref._u64(ref.comb(ref._obj(ev[1:]), [(cref.coef_ring(ci), list(Si)) for Si, ci in zip(sh[1], sh[2])]))      # sum_i c_i prod v_j, in Python integers
    rejected = 0
    for j in range(1, 1 + sh[0]):
        bad = dict(proof, evals=proof["evals"].copy())
        bad["evals"][j, 3] ^= np.uint64(1)
        moves = not np.array_equal(g(bad["evals"]), g(proof["evals"]))      # (v_j may cancel out of the identity: +M_1 f - M_1 f in shape c)
        ok, st, _ = plus.ccs_verify(_seeded(), _shape(sh), bad)
        assert (ok, st) == ((False, 2) if moves else (True, 0)), j
        rejected += moves
    assert rejected >= 1


_VAN = {}


def _vanishing_case(name, nvars):
    """a satisfied instance of shape `name`: every matrix is the identity and f holds the ring constants 0 / 1, so every g_j is the same idempotent table e
    (e * e = e) and every chain is e; the terms then sum to (sum_i c_i) e, and the LAST coefficient is replaced by minus the sum of the others (a general ring
    element wherever the shape has one).  -> (shape, f, mats, the reference's proof on the seeded oracle transcript)"""
    key = (name, nvars)
    if key not in _VAN:
        t, S, c = cref.shape(name)
        n = 1 << nvars
        rng = np.random.default_rng(0x7A + nvars)
        f = np.zeros((n, D), dtype=np.uint64)
        f[:, 0] = rng.integers(0, 2, size=n).astype(np.uint64)
        f[0, 0], f[n - 1, 0] = 1, 0
        ident = lfp.identity_csr(n)
        mats = [ident] * t
        cs = [cref.coef_ring(x).astype(object) for x in c]
        last = len(cs) - 1
        cs[last] = (-sum(cs[:last])) % P
        sh = (t, S, [np.array(x % P, dtype=object).astype(np.uint64) for x in cs])
        tr = lfp.Transcript()
        tr.absorb(ref.rand_ring(0x5EED, (2, D)))
        proof = cref.linearize(tr, sh, f, mats)
        _VAN[key] = (sh, f, mats, proof)
    return _VAN[key]


def _raw_verify(tr, nvars, t, q, off, idx, c, msgs, ev):
    off, idx = np.asarray(off, dtype=np.uint32), np.asarray(idx, dtype=np.uint32)
    c = np.ascontiguousarray(c, dtype=np.uint64)
    d = plus.CCSDesc(t, q, off.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), c.ctypes.data_as(u64p))
    ro, st = np.zeros(max(nvars, 1), dtype=np.uint64), C.c_int(-7)
    return plus._lib().lfplus_ccs_verify(tr.h, nvars, C.byref(d), msgs.ctypes.data_as(u64p), ev.ctypes.data_as(u64p), ro.ctypes.data_as(u64p), C.byref(st))


def test_verify_refusals_in_order():
    """every refusal of the envelope is LFPLUS_E_ARG and leaves the transcript untouched; an argument that breaks two rules is refused by the earlier one (seen
    through lfplus_last_error on a context in the GPU tests; here: each alone)"""
    L = plus._lib()
    sh, f, mats, proof = _vanishing_case("b", 3)
    nvars = 3
    msgs, ev = np.ascontiguousarray(proof["msgs"]), np.ascontiguousarray(proof["evals"])
    tr = _seeded()
    fresh = _seeded().get_challenge()
    t, S, c = sh
    off = np.concatenate([[0], np.cumsum([len(x) for x in S])])
    idx = np.concatenate(S)
    cw = np.stack(c)
    A = plus.E_ARG
    assert _raw_verify(tr, nvars, t, len(S), off, idx, cw, msgs, ev) == 0      # (the arrays as they are: accepted)
    tr = _seeded()
    d = _shape(sh).desc()
    ro, st = np.zeros(nvars, dtype=np.uint64), C.c_int()
    pm, pe, pr = msgs.ctypes.data_as(u64p), ev.ctypes.data_as(u64p), ro.ctypes.data_as(u64p)
    assert L.lfplus_ccs_verify(None, nvars, C.byref(d), pm, pe, pr, C.byref(st)) == A
    assert L.lfplus_ccs_verify(tr.h, nvars, None, pm, pe, pr, C.byref(st)) == A
    assert L.lfplus_ccs_verify(tr.h, nvars, C.byref(d), None, pe, pr, C.byref(st)) == A
    assert L.lfplus_ccs_verify(tr.h, nvars, C.byref(d), pm, None, pr, C.byref(st)) == A
    assert L.lfplus_ccs_verify(tr.h, nvars, C.byref(d), pm, pe, None, C.byref(st)) == A
    for bad in (plus.CCSDesc(t, len(S), None, d.S_idx, d.c), plus.CCSDesc(t, len(S), d.S_off, None, d.c), plus.CCSDesc(t, len(S), d.S_off, d.S_idx, None)):
        assert L.lfplus_ccs_verify(tr.h, nvars, C.byref(bad), pm, pe, pr, C.byref(st)) == A
    q = len(S)
    for tt, qq in ((0, q), (9, q), (t, 0), (t, 9)):
        assert _raw_verify(tr, nvars, tt, qq, off, idx, cw, msgs, ev) == A
    off1 = off.copy(); off1[0] = 1
    assert _raw_verify(tr, nvars, t, q, off1, idx, cw, msgs, ev) == A
    off2 = off.copy(); off2[2] = off2[1]                                        # an empty multiset
    assert _raw_verify(tr, nvars, t, q, off2, idx, cw, msgs, ev) == A
    assert _raw_verify(tr, nvars, 1, 1, [0, 8], [0] * 8, cw[:1], msgs, ev) == A  # eight indices in one multiset: d <= 7
    assert _raw_verify(tr, nvars, 1, 3, [0, 6, 12, 17], [0] * 17, cw[:3], msgs, ev) == A  # 17 indices in all
    idx2 = idx.copy(); idx2[-1] = t
    assert _raw_verify(tr, nvars, t, q, off, idx2, cw, msgs, ev) == A
    c2 = cw.copy(); c2[1, 15] = P
    assert _raw_verify(tr, nvars, t, q, off, idx, c2, msgs, ev) == A
    for nv in (0, 33):
        assert _raw_verify(tr, nv, t, q, off, idx, cw, msgs, ev) == A
    assert tr.get_challenge() == fresh, "a refused call leaves the transcript alone"
    assert L.lfplus_ccs_verify(_seeded().h, nvars, C.byref(d), pm, pe, pr, None) == 0      # (stage may be NULL)
    # the Python mirror: malformed proofs and shapes are E_ARG before the library is entered
    for bad in (dict(proof, msgs=proof["msgs"][:, :-1]), dict(proof, evals=proof["evals"][:-1]), dict(proof, nvars=0), {"nvars": 3}):
        with pytest.raises(plus.LfPlusError) as e:
            plus.ccs_verify(_seeded(), _shape(sh), bad)
        assert e.value.code == A
    with pytest.raises(plus.LfPlusError) as e:
        plus.ccs_verify(_seeded(), plus.CCSShape(9, [[0]], [1]), proof)
    assert e.value.code == A
    with pytest.raises(plus.LfPlusError) as e:
        plus.ccs_verify(_seeded(), (3, [[0, 1], [2]], [1, -1]), proof)
    assert e.value.code == A


def test_device_entry_points_without_a_context():
    """lfplus_ccs_linearize / lfplus_ccs_check with a NULL context are LFPLUS_E_ARG, as lfplus_r1cs_linearize / lfplus_r1cs_check are (without a device no context
    can exist: lfplus_ctx_create said LFPLUS_E_NO_DEVICE, and the wrapper ends there); the transcript is untouched"""
    import torch
    L = plus._lib()
    d = plus.CCSShape.r1cs().desc()
    tr = plus.PoseidonTranscript()
    fresh = plus.PoseidonTranscript().get_challenge()
    o = np.zeros(4 * 4 * D, dtype=np.uint64).ctypes.data_as(u64p)
    failed = C.c_uint()
    assert L.lfplus_ccs_linearize(None, tr.h, C.byref(d), None, None, None, o, o, o) == plus.E_ARG
    assert L.lfplus_r1cs_linearize(None, tr.h, None, None, None, o, o, o) == plus.E_ARG
    assert L.lfplus_ccs_check(None, None, C.byref(d), None, None, None, 0, C.byref(failed), None, None) == plus.E_ARG
    assert L.lfplus_r1cs_check(None, None, None, None, None, 0, C.byref(failed), None, None) == plus.E_ARG
    assert tr.get_challenge() == fresh
    if not torch.cuda.is_available():
        with pytest.raises(plus.LfPlusError) as e:
            plus.PlusContext(0)
        assert e.value.code == plus.E_NO_DEVICE
