"""The prover object of the C ABI for committed CCS instances (lfplus_prover_create_ccs, lfplus_prover_check_fresh, lfplus_verify_ccs: csrc/lfp_prover.cpp) on
the GPU.  Yardsticks, none of them the code under test: the R1CS prover object and the live oracle at the R1CS shape (the anchor), the parent's tested
ComCCS.linearize on separate contexts plus the oracle's cm_prove / decompose for a general shape, the Python-orchestrated plus.PlusProver(shape=) in the same
process for the chains, and the oracle's verifiers throughout.

Statements.  A CHAIN (cases 1, 3, 4, 5) runs at n = 2^15, kappa 1, k 4, B = estimate_bound / 2 -- tests/test_gpu_lfplus_native.py's chain statement.  The
fold test's k = 2 cannot carry a chain: the accumulator halves have norm up to B / 2 and two digits admit (d / 2)^2 = 64, so the SECOND proof of any chain is
rejected by the oracle's verifier and by lfplus_verify alike (cm stage 5), whatever produced it; k = 4 then needs n = 2^15 (kappa k d l d < n).  The one-prove
case 2 keeps the fold test's parameters (nvars 14, kappa 1, k 2, B = estimate_bound(16 128, L, 16, k) + 1).
Satisfied instances: binary z (constant coefficient 0 / 1, so z^m = z) under t copies of pad_rows(gadget_decompose_csr(identity, B, k)), coefficients that
cancel.  Case 2 uses DISTINCT random matrices instead (nothing there needs a satisfied instance): a confusion of matrix indices shows there."""
import ctypes as C

import numpy as np
import pytest

import lfp
import lfplus_ccs_ref as cref
import lfplus_mlsumcheck_ref as ref
import test_gpu_lfplus_native as nat
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
P, D = plus.P, plus.D
N = nat.N
KAPPA, K, ROUNDS = 1, 4, (2, 1, 1)
CM_KEYS = ("msgs", "r", "e", "b", "v", "a", "bb", "c", "comh", "pa", "ea", "pb", "eb", "ro", "cm_g", "vo")


def _g(seed):
    return ref.rand_ring(0xCC5 + seed, (D,))


def _neg(g):
    return np.where(g == 0, np.uint64(0), np.uint64(P) - g)


SHAPES = {
    "deg3": (4, [[0, 1, 2], [3]], [1, -1]),
    "gate4": (4, cref.shape("b4")[1], [_g(2), _neg(_g(2)), 5, -5, 0]),      # both general-coefficient chains, the zero term dropped
    "wide": (8, [[0, 1, 2, 3, 4, 5, 6], [7, 0]], [_g(9), _neg(_g(9))]),    # the full envelope: t = 8, d = 7
}


def _statement(name):
    sh = SHAPES[name]
    A, r1cs, params = nat._shape(KAPPA, K)
    return sh, plus.CCSShape(*sh), A, [r1cs[0]] * sh[0], params


def _header(sh, params, nvars, L, nfresh):
    t, S, _ = sh
    dp = params.lin.decomp
    return [int.from_bytes(b"LFPLUS02", "big"), L, nfresh, nvars, dp.k, dp.l, params.lin.kappa, t, len(S), max(len(x) for x in S), sum(len(x) for x in S), 0]


def _commit_all(A, fs):
    c = plus.PlusContext(0)
    try:
        c.set_matrix(A)
        return [c.commit(f) for f in fs]
    finally:
        c.close()


def _raw_check_fresh(prover, count, bound=0):
    ok, failed, fb, am = (C.c_int * count)(), (C.c_uint * count)(), (C.c_uint64 * count)(), (C.c_uint64 * count)()
    rc = plus._nlib().lfplus_prover_check_fresh(prover.h, bound, ok, failed, fb, am)
    return rc, [(ok[i], failed[i], fb[i], am[i]) for i in range(count)]


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------------------------------------
def test_anchor_the_r1cs_shape_equals_the_r1cs_prover_object_and_the_live_oracle():
    """the CCS prover at t = 3, S = ({0,1},{2}), c = (1, -1) on the chain (2, 1, 1) next to the lfplus_prover_create prover on the same inputs and the live
    oracle: every word after the header, the accumulator after each round, the closing challenge; lfplus_verify_ccs and the oracle's verifier accept.
    (The oracle's chain is nat._oracle's, computed once per process on the CPU -- about 14 s -- and shared with tests/test_gpu_lfplus_native.py, which then finds it
    cached: nothing is added to the suite.)"""
    A, r1cs, params = nat._shape(KAPPA, K)
    runs, closing = nat._oracle(KAPPA, K, ROUNDS)
    sh = plus.CCSShape.r1cs()
    pc = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript(), shape=sh)
    pr = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    ver, ts_o = plus.NativePlusVerifier.init(A, list(r1cs), params, plus.PoseidonTranscript(), shape=sh), lfp.Transcript()
    try:
        nacc = 0
        for zs, (want, want_acc) in zip(nat._zs(K, ROUNDS), runs):
            pc.ingest(zs)
            pr.ingest(zs, r1cs)
            assert pc.check_fresh(params.B) == pr.check_fresh(params.B) and all(x[:3] == (True, 0, N) for x in pc.check_fresh())
            fc, fr = pc.prove(), pr.prove()
            L, nfresh = nacc + len(zs), len(zs)
            assert fc.size == fr.size + 4 == plus.proof_len(params, N, None, L, nfresh, shape=sh)
            assert [int(x) for x in fc[:12]] == _header(cref.R1CS, params, 15, L, nfresh)
            assert np.array_equal(fc[12:], fr[8:])
            got = plus.proof_from_flat(fc, params, N, None, L, nfresh, shape=sh)
            nat._same_proof(got, want, nfresh, f"round L={L}")
            ac, ar = pc.accumulator(), pr.accumulator()
            for i in range(2):
                assert np.array_equal(ac[i], want_acc[i]) and np.array_equal(ar[i], want_acc[i])
            assert pc.decide(fc, params.B) == pr.decide(fr, params.B) and all(x[:2] == (True, 0) for x in pc.decide(fc, params.B))
            assert ver.verify(fc, L, nfresh), ver.stage
            assert lfp.plus_verify(ts_o, got, params.B) == 0
            nacc = 2
        assert pc.transcript.get_challenge() == closing == ver.transcript.get_challenge() == pr.transcript.get_challenge()
    finally:
        pc.close()
        pr.close()
        plus.scratch_trim(0)


# ---- 2. a general shape against the live oracle ---------------------------------------------------------------------------------------------------------------
def _small_witness(n, seed):
    v = (lfp.splitmix(seed, 0, n * D) % np.uint64(63)).astype(np.int64) - 31
    return np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64)).reshape(n, D)


def _seeded(cls):
    t = cls()
    t.absorb(ref.rand_ring(0x5EED, (2, D)))
    return t


def test_deg3_one_prove_of_two_instances_equals_the_parents_linearize_and_the_oracles_fold():
    """deg3, nfresh = L = 2 at the fold test's parameters: the linearization fields equal ComCCS.linearize on separate contexts, the oracle transcript follows by
    cref.replay, and EVERY CmProof field, the LinB2X and the DecompProof fields equal lfp.cm_prove / lfp.decompose word for word; (F0, F1) are the accumulator.
    The only case that pays for the oracle's cm_prove with four matrices (1.9 s per instance on a CPU)."""
    nvars, kappa, k, Lq = 14, 1, 2, 2
    n = 1 << nvars
    B = plus.estimate_bound(16 * 128, Lq, D, k) + 1
    dp = plus.DecompParameters.for_frog(k)
    params = plus.PlusParameters(plus.LinParameters(kappa, dp), B)
    sh = SHAPES["deg3"]
    shape = plus.CCSShape(*sh)
    A = lfp.splitmix(3, 0, kappa * n * D).reshape(kappa, n, D) % np.uint64(P)
    mats = []
    for j in range(4):      # distinct, constant coefficients (the range relation needs them), small ones
        rp, col, val = ref.rand_csr(0x70 + j, n, 1)
        val = val.copy()
        val[:, 1:] = 0
        val[:, 0] %= np.uint64(5)
        mats.append((rp, col, val))
    fs = [_small_witness(n, 40 + l) for l in range(Lq)]
    prover = plus.NativePlusProver.init(A, mats, 0, params, _seeded(plus.PoseidonTranscript), shape=shape)
    ctxs = []
    try:
        prover.set_instances(fs)
        chk = prover.check_fresh()
        assert all(not ok and failed == plus.REL_CCS and fb < n for ok, failed, fb, _ in chk), chk      # random instances are not satisfied: nothing below needs them to be
        flat = prover.prove()
        assert flat.size == plus.proof_len(params, n, None, Lq, Lq, shape=shape) and [int(x) for x in flat[:12]] == _header(sh, params, nvars, Lq, Lq)
        got = plus.proof_from_flat(flat, params, n, None, Lq, Lq, shape=shape)
        tr, tr_o = _seeded(plus.PoseidonTranscript), _seeded(lfp.Transcript)
        for l in range(Lq):
            c = plus.PlusContext(0)
            ctxs.append(c)
            c.set_matrix(A)
            _, proof = plus.ComCCS(shape, tuple(mats), fs[l], None).linearize(c, tr)
            for key in ("msgs", "r", "evals"):
                assert np.array_equal(got["lproof"][l][key], proof[key]), (l, key)
            cref.replay(tr_o, sh, proof)
        verifier_o = tr_o.clone()
        insts = []
        for f in fs:
            rg = lfp.rg_from_f(f, A, dp.b, dp.k, dp.l)
            tau_i = np.array([int(t) if int(t) <= P // 2 else int(t) - P for t in rg["tau"]], dtype=np.int8)
            insts.append({"Mf": lfp.exp_dense(rg["Df"]), "tau": rg["tau"], "mtau": lfp.exp_dense(tau_i), "f": f, "comMf": rg["comMf"],
                          "fcoms": np.stack([rg["cm_f"], rg["C_Mf"], rg["cm_mtau"]])})
        want = lfp.cm_prove(tr_o, nvars, insts, k, dp.l, kappa, mats)
        cm = got["cmproof"]
        for key in CM_KEYS:
            assert np.array_equal(cm[key], want[key]), key
        assert np.array_equal(cm["fcoms"], np.stack([i["fcoms"] for i in insts]))
        g, cm_g, vo = want["g"][0], want["cm_g"][0], want["vo"][0]
        for i in range(1, Lq):
            g, cm_g, vo = lfp.addmod(g, want["g"][i]), lfp.addmod(cm_g, want["cm_g"][i]), lfp.addmod(vo, want["vo"][i])
        x = got["linb2x"]
        assert np.array_equal(x["cm_g"], cm_g) and np.array_equal(x["vo"], vo) and np.array_equal(x["ro"], want["ro"])
        r_pairs = plus._ro_pairs(x["ro"])
        wd = lfp.decompose(g, A, B, np.ascontiguousarray(r_pairs[:, 0]), np.ascontiguousarray(r_pairs[:, 1]), mats)
        for key in ("C0", "C1", "v0", "v1"):
            assert np.array_equal(got["dproof"][key], wd[key]), key
        acc = prover.accumulator()
        assert np.array_equal(acc[0], wd["F0"]) and np.array_equal(acc[1], wd["F1"])
        assert prover.transcript.get_challenge() == tr_o.challenge()
        assert lfp.cm_verify(verifier_o, cm, list(cm["fcoms"]))[0] == 0
        assert lfp.decomp_verify(got["dproof"], cm_g, vo, B) == 0
        assert all(r[:2] == (True, 0) for r in prover.decide(flat, B))
        # the verifier object sees what check_fresh saw: instance 0 does not sum to zero
        ver = plus.NativePlusVerifier.init(A, mats, params, _seeded(plus.PoseidonTranscript), shape=shape)
        assert not ver.verify(flat, Lq, Lq) and ver.code == plus.E_REJECT and ver.which == 0 and ver.stage == ("lproof[0]", 1)
    finally:
        for c in ctxs:
            c.close()
        prover.close()
        plus.scratch_trim(0)


# ---- 3. chains -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deg3", "gate4", "wide"])
def test_chains_native_equals_python_in_both_input_forms_and_every_verifier_accepts(name):
    """rounds (2, 1, 1), i.e. L = 2, 3, 3 with the accumulator resident from the previous prove: the native flat proofs of the ingest (z) form equal those of the
    set_instances (f, cm_f) form and proof_to_flat of plus.PlusProver(shape=); check_fresh reports every instance satisfied, decide both halves valid under
    the norm bound B; lfplus_verify_ccs accepts each proof on one running transcript, and so do the oracle's cm_verify / decomp_verify behind cref.replay"""
    sh, shape, A, M, params = _statement(name)
    zs_all = nat._zs(K, ROUNDS)

    def native(host):
        prover = plus.NativePlusProver.init(A, M, 1, params, plus.PoseidonTranscript(), shape=shape)
        try:
            out = []
            for zs in zs_all:
                if host:
                    fs = [plus.gadget_decompose(z, params.B, K) for z in zs]
                    prover.set_instances(fs, _commit_all(A, fs))
                else:
                    prover.ingest(zs)
                chk = prover.check_fresh(params.B)
                assert len(chk) == len(zs) and all(ok and failed == 0 and fb == N and 1 <= am < params.B for ok, failed, fb, am in chk), chk
                flat = prover.prove()
                dec = prover.decide(flat, params.B)
                assert all(ok and failed == 0 and am < params.B for ok, failed, am in dec), dec
                out.append((flat, prover.accumulator()))
            return out, prover.transcript.get_challenge()
        finally:
            prover.close()

    def python():
        prover = plus.PlusProver.init(A, M, 1, params, plus.PoseidonTranscript(), shape=shape)
        prover.device_acc = True
        try:
            out = []
            for zs in zs_all:
                out.append((plus.proof_to_flat(prover.prove(prover.ingest(zs)), params, N, None, shape=shape), prover.accumulator()))
            return out, prover.transcript.get_challenge()
        finally:
            prover.close()
    try:
        got, closing = native(False)
        for form, (other, ch) in (("host form", native(True)), ("python", python())):
            assert ch == closing, form
            for (fa, aa), (fb, ab) in zip(got, other):
                assert fa.shape == fb.shape and np.array_equal(fa, fb), form
                assert np.array_equal(aa[0], ab[0]) and np.array_equal(aa[1], ab[1]), form
        ver, tr_o, nacc = plus.NativePlusVerifier.init(A, M, params, plus.PoseidonTranscript(), shape=shape), lfp.Transcript(), 0
        for zs, (flat, _) in zip(zs_all, got):
            L, nfresh = nacc + len(zs), len(zs)
            assert [int(x) for x in flat[:12]] == _header(sh, params, 15, L, nfresh)
            assert ver.verify(flat, L, nfresh), (L, ver.stage)
            proof = plus.proof_from_flat(flat, params, N, None, L, nfresh, shape=shape)
            for lp in proof["lproof"]:
                assert lp["msgs"].shape == (15, shape.degree + 2, D) and lp["evals"].shape == (1 + shape.t, D)
                cref.replay(tr_o, sh, lp)
            rc, x = lfp.cm_verify(tr_o, proof["cmproof"], list(proof["cmproof"]["fcoms"]))
            assert rc == 0
            assert np.array_equal(x["cm_g"], proof["cmproof"]["cm_g"]) and np.array_equal(x["vo"], proof["cmproof"]["vo"])
            assert lfp.decomp_verify(proof["dproof"], proof["linb2x"]["cm_g"], proof["linb2x"]["vo"], params.B) == 0
            nacc = 2
        assert ver.transcript.get_challenge() == closing == tr_o.challenge()
    finally:
        plus.scratch_trim(0)


# ---- 4. rejection ----------------------------------------------------------------------------------------------------------------------------------------------
def test_an_unsatisfied_instance_is_reported_by_check_fresh_proved_anyway_and_rejected_by_the_verifier():
    """bit 1 of one constant coefficient of one z is set (the entry becomes 2 or 3: z^3 != z in that row).  check_fresh: LFPLUS_E_REJECT, LFPLUS_REL_CCS and that
    row for that instance alone; the prover stays usable and proves (the reference does not check either); lfplus_verify_ccs rejects with which = that instance.
    The same z under the R1CS prover object: LFPLUS_REL_R1CS at that row.  A wrong cm_f given to set_instances: reported, and it fails the prove, as for R1CS."""
    sh, shape, A, M, params = _statement("deg3")
    zs = [z.copy() for z in nat._zs(K, ROUNDS)[0]]
    row = 4321
    zs[1][row, 0] ^= np.uint64(2)
    prover = plus.NativePlusProver.init(A, M, 1, params, plus.PoseidonTranscript(), shape=shape)
    try:
        prover.ingest(zs)
        ch0 = prover.transcript.clone().get_challenge()
        rc, out = _raw_check_fresh(prover, 2, params.B)
        assert rc == plus.E_REJECT and out[0][:3] == (1, 0, N) and out[1][:3] == (0, plus.REL_CCS, row), out
        assert prover.check_fresh() == [(True, 0, N, out[0][3]), (False, plus.REL_CCS, row, out[1][3])]
        assert prover.transcript.clone().get_challenge() == ch0           # read-only: the transcript has not moved
        flat = prover.prove()
        ver = plus.NativePlusVerifier.init(A, M, params, plus.PoseidonTranscript(), shape=shape)
        assert not ver.verify(flat, 2, 2) and ver.code == plus.E_REJECT and ver.which == 1 and ver.stage == ("lproof[1]", 1)
        with pytest.raises(plus.LfPlusError) as e:                       # after the prove: no fresh instances
            prover.check_fresh()
        assert e.value.code == plus.E_ARG
    finally:
        prover.close()
    # the call changes nothing: a prover that was never asked writes the same proof
    quiet = plus.NativePlusProver.init(A, M, 1, params, plus.PoseidonTranscript(), shape=shape)
    try:
        quiet.ingest(zs)
        assert np.array_equal(quiet.prove(), flat)
    finally:
        quiet.close()
    _, r1cs, _ = nat._shape(KAPPA, K)
    pr = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        pr.ingest(zs, r1cs)
        rc, out = _raw_check_fresh(pr, 2)
        assert rc == plus.E_REJECT and out[0][:3] == (1, 0, N) and out[1][:3] == (0, plus.REL_R1CS, row), out
    finally:
        pr.close()
    # a wrong commitment
    good = nat._zs(K, ROUNDS)[0]
    fs = [plus.gadget_decompose(z, params.B, K) for z in good]
    cms = _commit_all(A, fs)
    cms[0] = cms[0].copy()
    cms[0][0, 3] = (int(cms[0][0, 3]) + 1) % P
    prover = plus.NativePlusProver.init(A, M, 1, params, plus.PoseidonTranscript(), shape=shape)
    try:
        prover.set_instances(fs, cms)
        chk = prover.check_fresh()
        assert chk[0][:3] == (False, plus.REL_CM, N) and chk[1][:3] == (True, 0, N), chk
        with pytest.raises(plus.LfPlusError) as e:
            prover.prove()
        assert e.value.code == plus.E_ARG and "cm_f" in str(e.value)
        with pytest.raises(plus.LfPlusError) as e:                       # a failed prover refuses check_fresh
            prover.check_fresh()
        assert e.value.code == plus.E_ARG and "failed earlier" in str(e.value)
    finally:
        prover.close()
        plus.scratch_trim(0)


# ---- 5. state machine and refusals -----------------------------------------------------------------------------------------------------------------------------
def test_state_machine_and_refusals():
    sh, shape, A, M, params = _statement("deg3")
    lib = plus._nlib()
    zs = nat._zs(K, ROUNDS)[0]
    plus.scratch_trim(0)
    before = plus.scratch_bytes(0)
    # a refused shape: *out = NULL and no context was built (nothing reached the scratch cache, nothing to destroy)
    keep, rp, cp, vp = plus._csr_args(M)
    ap = np.ascontiguousarray(A, dtype=np.uint64).ctypes.data_as(plus.u64p)
    tr = plus.PoseidonTranscript()
    for bad in (plus.CCSShape(4, [[0, 1, 4], [3]], [1, -1]), plus.CCSShape(4, [[0] * 8, [3]], [1, -1]), plus.CCSShape(4, [[0, 1, 2], [3]], [1, [P] + [0] * 15])):
        h = C.c_void_p(0xDEAD)
        d = bad.desc()
        assert lib.lfplus_prover_create_ccs(0, C.byref(plus._cparams(params)), ap, 0, N, C.byref(d), rp, cp, vp, 1, tr.h, C.byref(h)) == plus.E_ARG and h.value is None
    assert plus.scratch_bytes(0) == before
    with pytest.raises(plus.LfPlusError) as e:                           # the Python prover: a shape together with shard, before a context exists
        plus.PlusProver.init(A, M, 1, params, tr, shard=(0, 2, "model"), shape=shape)
    assert e.value.code == plus.E_ARG and plus.scratch_bytes(0) == before
    prover = plus.NativePlusProver.init(A, M, 1, params, tr, shape=shape)
    try:
        with pytest.raises(plus.LfPlusError) as e:                       # before any instances
            prover.check_fresh()
        assert e.value.code == plus.E_ARG and "no fresh instances" in str(e.value)
        prover.ingest(zs)
        ch0 = tr.clone().get_challenge()
        words3 = plus.proof_len(params, N, 3, 2, 2)                      # the R1CS layout's length on a CCS prover: refused, nothing touched
        buf = np.zeros(words3, dtype=np.uint64)
        assert lib.lfplus_prover_prove(prover.h, buf.ctypes.data_as(plus.u64p), words3) == plus.E_ARG and "proof_words" in prover.last_error()
        assert not buf.any() and tr.clone().get_challenge() == ch0
        assert all(x[0] for x in prover.check_fresh())                   # still named, still usable
        flat = prover.prove()
        assert plus.NativePlusVerifier.init(A, M, params, plus.PoseidonTranscript(), shape=shape).verify(flat, 2, 2)
        with pytest.raises(plus.LfPlusError) as e:                       # after the prove
            prover.check_fresh()
        assert e.value.code == plus.E_ARG
        # decide with a proof of another shape: the R1CS layout's length, a shorter buffer, and the right length under a header that names another q
        other = plus.CCSShape(4, [[0, 1, 2], [3], [3]], [1, -1, 0])
        wrong = flat.copy()
        wrong[8] = 3
        assert plus.proof_len(params, N, None, 2, 2, shape=other) == flat.size
        for w in (np.zeros(words3, dtype=np.uint64), flat[4:].copy(), wrong):
            with pytest.raises(plus.LfPlusError) as e:
                prover.decide(w, params.B)
            assert e.value.code == plus.E_ARG and "not the flat proof" in str(e.value)
        assert all(x[:2] == (True, 0) for x in prover.decide(flat, params.B))
        with pytest.raises(plus.LfPlusError) as e:                       # capacity after the first prove: ncomp = 1
            prover.ingest(zs)
        assert e.value.code == plus.E_ARG
        with pytest.raises(plus.LfPlusError) as e:                       # a CCS prover of the Python form takes ComCCS, the R1CS one ComR1CS: checked before anything moves
            pp = plus.PlusProver.init(A, M, 1, params, plus.PoseidonTranscript(), shape=shape)
            try:
                pp.prove([plus.ComR1CS(tuple(M[:3]), zs[0], plus.gadget_decompose(zs[0], params.B, K), None)])
            finally:
                assert pp.failed is None
                pp.close()
        assert e.value.code == plus.E_ARG
    finally:
        prover.close()
    plus.scratch_trim(0)
    assert plus.scratch_bytes(0) == before
