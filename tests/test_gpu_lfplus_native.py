"""PlusProver / PlusVerifier as objects of the C ABI (lfplus_prover_*, lfplus_verify: csrc/lfp_prover.cpp) on the GPU, and the seeded commitment matrix
(lfplus_matrix_generate, k_fill_ajtai).  The yardsticks are the live oracle (lfp.PlusOracle on the shapes of tests/test_gpu_lfplus_prover.py, computed
once per process), the Python-orchestrated plus.PlusProver in the same process, and the committed P15 digests."""
import ctypes as C
from math import ceil, log

import numpy as np
import pytest

import lfp
import test_gpu_lfplus_prover as base
from test_gpu_lfplus_scale import digests, gold
from latticefold_amd import plus

pytestmark = pytest.mark.gpu
D, P = 16, plus.P
N, ELL = 1 << 15, ceil(log(P) / log(8))


def _shape(kappa, k):
    """the statement of base.test_plus_prover_matches_oracle: (A, r1cs, params)"""
    B = base._bound(3, k) + 1 if k == 2 else base._bound(3, k) // 2
    A = lfp.splitmix(23, 0, kappa * N * D).reshape(kappa, N, D)
    r1cs = plus.r1cs_decomposed_square((plus.identity_csr(N // k),) * 3, N, B, k)
    return A, r1cs, plus.PlusParameters(plus.LinParameters(kappa, plus.DecompParameters(8, k, ELL)), B)


def _zs(k, rounds):
    rng, out = np.random.default_rng(8), []
    for ncomp in rounds:
        zs = []
        for _ in range(ncomp):
            z = np.zeros((N // k, D), dtype=np.uint64)
            z[:, 0] = rng.integers(0, 2, size=N // k)
            zs.append(z)
        out.append(zs)
    return out


_ORACLE = {}


def _oracle(kappa, k, rounds):
    """the oracle's proofs, accumulators and closing challenge of one shape, computed once per process for the tests of this module"""
    case = (kappa, k, rounds)
    if case not in _ORACLE:
        A, r1cs, params = _shape(kappa, k)
        oracle = lfp.PlusOracle(A, list(r1cs), kappa, 8, k, ELL, params.B, lfp.Transcript())
        runs = []
        for zs in _zs(k, rounds):
            want = oracle.prove([(lfp.gadget_decompose(z, params.B, k), r1cs) for z in zs])
            runs.append((want, [np.array(a, copy=True) for a in oracle.acc]))
        _ORACLE[case] = (runs, oracle.tr.challenge())
    return _ORACLE[case]


def _same_proof(got, want, nfresh, where):
    for i in range(nfresh):
        base._same(got["lproof"][i], want["lproof"][i], ("msgs", "r", "evals"), f"{where} lproof[{i}]")
    base._same(got["cmproof"], want["cmproof"], base.CM_KEYS, f"{where} cmproof")
    base._same(got["linb2x"], want["linb2x"], ("cm_g", "ro", "vo"), f"{where} linb2x")
    base._same(got["dproof"], want["dproof"], ("C0", "C1", "v0", "v1"), f"{where} dproof")


@pytest.mark.parametrize("kappa,k,rounds", [(2, 2, (2,)), (1, 4, (2, 1, 1))])
def test_native_prover_matches_the_live_oracle(kappa, k, rounds):
    """every proof field word for word through proof_from_flat, the accumulator after each round, the closing challenge; lfplus_verify and the oracle's
    verifier accept each proof on one running transcript"""
    A, r1cs, params = _shape(kappa, k)
    runs, closing = _oracle(kappa, k, rounds)
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    ver, ts_o = plus.NativePlusVerifier.init(A, list(r1cs), params, plus.PoseidonTranscript()), lfp.Transcript()
    try:
        nacc = 0
        for zs, (want, want_acc) in zip(_zs(k, rounds), runs):
            cm = prover.ingest(zs, r1cs)
            flat = prover.prove()
            L, nfresh = nacc + len(zs), len(zs)
            assert prover.last == (L, nfresh) and flat.size == plus.proof_len(params, N, 3, L, nfresh)
            got = plus.proof_from_flat(flat, params, N, 3, L, nfresh)
            _same_proof(got, want, nfresh, f"round L={L}")
            for i in range(nfresh):
                assert (cm[i] == want["cmproof"]["fcoms"][nacc + i][0]).all()
            acc = prover.accumulator()
            for i in range(2):
                assert (acc[i] == want_acc[i]).all()
            assert ver.verify(flat, L, nfresh), ver.stage
            assert lfp.plus_verify(ts_o, got, params.B) == 0
            nacc = 2
        assert prover.transcript.get_challenge() == closing == ver.transcript.get_challenge()
    finally:
        prover.close()
        plus.scratch_trim(0)


def test_ingest_form_equals_host_form_equals_the_python_prover():
    """one chain (kappa 1, k 4, rounds (2, 1)) through NativePlusProver.ingest(z), through NativePlusProver.set_instances(f, cm_f) -- the witnesses go up on
    the library's worker thread -- and through plus.PlusProver (device_acc, ingest) in the same process: identical flat proofs, accumulators and challenges"""
    kappa, k, rounds = 1, 4, (2, 1)
    A, r1cs, params = _shape(kappa, k)
    zs_all = _zs(k, rounds)

    def native(host):
        prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
        try:
            out = []
            for zs in zs_all:
                if host:
                    fs = [plus.gadget_decompose(z, params.B, k) for z in zs]
                    scratch = plus.PlusContext(0)
                    try:
                        scratch.set_matrix(A)
                        cms = [scratch.commit(f) for f in fs]
                    finally:
                        scratch.close()
                    prover.set_instances(fs, cms)
                else:
                    prover.ingest(zs, r1cs)
                flat = prover.prove()
                out.append((flat, prover.accumulator()))
            return out, prover.transcript.get_challenge()
        finally:
            prover.close()

    def python():
        prover = plus.PlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
        prover.device_acc = True
        try:
            out = []
            for zs in zs_all:
                out.append((plus.proof_to_flat(prover.prove(prover.ingest(zs, r1cs)), params, N, 3), prover.accumulator()))
            return out, prover.transcript.get_challenge()
        finally:
            prover.close()
    try:
        ref, ref_ch = native(False)
        for name, (got, ch) in (("host form", native(True)), ("python", python())):
            assert ch == ref_ch, name
            for (fa, aa), (fb, ab) in zip(ref, got):
                assert fa.shape == fb.shape and (fa == fb).all(), name
                assert (aa[0] == ab[0]).all() and (aa[1] == ab[1]).all(), name
    finally:
        plus.scratch_trim(0)


def test_native_prove_reproduces_the_p15_fixture_from_a_seeded_matrix():
    """P15 (three fresh instances in one prove): the native prover with A = NULL (the matrix generated on the device from the workload's seed) reproduces
    every digest of tests/golden/lfplus_digests.json["P15"]; a native prover given the host matrix writes the same words; lfplus_verify accepts them"""
    want = gold("P15")
    wl = plus.make_plus_workload("P15")
    r1cs, params = wl.r1cs(), wl.params()
    zs = [wl.z(i) for i in range(wl.L)]
    out = []
    try:
        for A in (None, wl.ajtai_matrix()):
            prover = plus.NativePlusProver.init(A, list(r1cs), max(1, wl.L - 2), params, plus.PoseidonTranscript(), seed=wl.ajtai_seed)
            try:
                prover.ingest(zs, r1cs)
                flat = prover.prove()
                out.append((flat, prover.accumulator(), prover.transcript.get_challenge()))
            finally:
                prover.close()
        flat, acc, ch = out[0]
        got = digests(plus.proof_from_flat(flat, params, wl.n, 3, wl.L, wl.L), acc, ch)
        bad = [key for key in want if got.get(key) != want[key]]
        assert not bad, f"P15: fields differing from the oracle fixture: {bad}"
        assert (out[1][0] == flat).all() and out[1][2] == ch and all((a == b).all() for a, b in zip(out[1][1], acc))
        ver = plus.NativePlusVerifier.init((wl.kappa, wl.n, D), list(r1cs), params, plus.PoseidonTranscript())
        assert ver.verify(flat, wl.L, wl.L), ver.stage
    finally:
        plus.scratch_trim(0)


def test_decide_checks_the_accumulator_where_it_lives_and_changes_nothing():
    kappa, k = 2, 2
    A, r1cs, params = _shape(kappa, k)
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        prover.ingest(_zs(k, (2,))[0], r1cs)
        flat = prover.prove()
        keep, acc = flat.copy(), prover.accumulator()
        am = [int(np.abs(plus._centre(acc[i])).max()) for i in range(2)]      # the largest |centred word| of each half, from the read-back accumulator
        assert 1 <= am[0] < params.B and am[1] < params.B
        res = prover.decide(flat, params.B)
        assert res == [(True, 0, am[0]), (True, 0, am[1])], res
        assert prover.decide(flat) == res                 # bound 0: the norm is not checked
        res = prover.decide(flat, 1)                      # ||F_i||_inf < 1 fails for every half that is not zero (F1 is zero when g fits one base-B digit)
        assert res == [(am[i] < 1, 0 if am[i] < 1 else plus.REL_NORM, am[i]) for i in range(2)] and not res[0][0], res
        bad = flat.copy()                                 # a wrong v0 word: the evaluation component of half 0 alone
        off, _ = plus.proof_layout(params, N, 3, 2, 2)
        bad[off[-2] + 3] = (int(bad[off[-2] + 3]) + 1) % P
        res = prover.decide(bad, params.B)
        assert res[0][:2] == (False, plus.REL_V) and res[1][:2] == (True, 0), res
        with pytest.raises(plus.LfPlusError) as e:        # not this prover's last proof: refused, not read
            prover.decide(flat[:-1], params.B)
        assert e.value.code == plus.E_ARG
        acc2 = prover.accumulator()
        assert (flat == keep).all() and (acc2[0] == acc[0]).all() and (acc2[1] == acc[1]).all()
    finally:
        prover.close()
        plus.scratch_trim(0)


def test_state_machine_capacity_failure_and_scratch():
    kappa, k, rounds = 2, 2, (2,)
    A, r1cs, params = _shape(kappa, k)
    runs, closing = _oracle(kappa, k, rounds)
    zs = _zs(k, rounds)[0]
    plus.scratch_trim(0)
    before = plus.scratch_bytes(0)
    # one more instance than contexts (2 + ncomp = 3): LFPLUS_E_ARG, nothing touched -- the prove that follows matches the oracle
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        for call in (lambda: prover.ingest(zs * 2, r1cs), lambda: prover.set_instances([np.zeros((N, D), dtype=np.uint64)] * 4)):
            with pytest.raises(plus.LfPlusError) as e:
                call()
            assert e.value.code == plus.E_ARG and "more instances than contexts" in str(e.value)
        with pytest.raises(plus.LfPlusError) as e:      # nothing named yet: nothing to fold, and still no failure
            prover.prove()
        assert e.value.code == plus.E_ARG
        with pytest.raises(plus.LfPlusError) as e:      # a shape error (m k != n) is refused before a context is touched: no failure either
            prover.ingest([z[:-1] for z in zs], r1cs)
        assert e.value.code == plus.E_ARG and "m * k" in str(e.value)
        prover.ingest(zs, r1cs)
        with pytest.raises(plus.LfPlusError) as e:      # the next prove has its instances already
            prover.ingest(zs, r1cs)
        assert e.value.code == plus.E_ARG
        flat = prover.prove()
        _same_proof(plus.proof_from_flat(flat, params, N, 3, 2, 2), runs[0][0], 2, "after the refusals")
        assert prover.transcript.get_challenge() == closing
        with pytest.raises(plus.LfPlusError) as e:      # capacity after the first prove: ncomp = 1
            prover.ingest(zs, r1cs)
        assert e.value.code == plus.E_ARG
    finally:
        prover.close()
    # a non-canonical z word: ingest fails, the prover is failed -- prove and ingest refuse, last_error says why; destroy leaks no scratch
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        bad = zs[1].copy()
        bad[N // k - 1, D - 1] = np.uint64(P)
        with pytest.raises(plus.LfPlusError) as e:
            prover.ingest([zs[0], bad], r1cs)
        assert e.value.code == plus.E_ARG and "non-canonical" in str(e.value)
        lib = plus._nlib()
        buf = np.zeros(plus.proof_len(params, N, 3, 2, 2), dtype=np.uint64)
        assert lib.lfplus_prover_prove(prover.h, buf.ctypes.data_as(plus.u64p), buf.size) == plus.E_ARG
        assert "failed earlier" in prover.last_error() and "non-canonical" in prover.last_error()
        with pytest.raises(plus.LfPlusError) as e:
            prover.ingest(zs, r1cs)
        assert e.value.code == plus.E_ARG and prover.last_error()
        with pytest.raises(plus.LfPlusError):
            prover.accumulator()
        assert not buf.any()
    finally:
        prover.close()
    # a host witness with a non-canonical word surfaces in the prove (the upload thread saw it) and fails the prover too
    prover = plus.NativePlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    try:
        fs = [plus.gadget_decompose(z, params.B, k) for z in zs]
        fs[1][5, 5] = np.uint64(P)
        prover.set_instances(fs)
        with pytest.raises(plus.LfPlusError) as e:
            prover.prove()
        assert e.value.code == plus.E_ARG and "non-canonical" in str(e.value)
        with pytest.raises(plus.LfPlusError) as e:
            prover.prove()
        assert "failed earlier" in str(e.value)
    finally:
        prover.close()
    assert plus.scratch_bytes(0) > before                 # (the destroyed contexts' blocks are in the process-wide cache ...)
    plus.scratch_trim(0)
    assert plus.scratch_bytes(0) == before                # (... and go back to the driver: nothing else is held)


@pytest.mark.parametrize("kappa,n", [(2, 1 << 12), (3, 1 << 10)])
def test_seeded_matrix_equals_the_host_stream(kappa, n):
    """A context filled by generate_matrix(seed) and one given the host words of the same stream (PlusWorkload.ajtai_matrix's recipe) return identical
    lfplus_commit results for e_0 and e_{n-1} (column 0 and the last column of A), e_{n/2-1} and e_{n/2}, and a random canonical vector"""
    seed = 0xA17A2 + 77
    host = np.stack([plus._splitmix_words(seed, i * n * D, n * D) % np.uint64(P) for i in range(kappa)]).reshape(kappa, n, D)
    rng = np.random.default_rng(4)
    vecs = []
    for col in (0, n - 1, n // 2 - 1, n // 2):
        v = np.zeros((n, D), dtype=np.uint64)
        v[col, 0] = 1
        vecs.append(v)
    vecs.append(rng.integers(0, P, size=(n, D), dtype=np.uint64))
    a, b = plus.PlusContext(0), plus.PlusContext(0)
    try:
        a.generate_matrix(seed, kappa, n)
        b.set_matrix(host)
        for j, v in enumerate(vecs):
            ca, cb = a.commit(v), b.commit(v)
            assert (ca == cb).all(), j
            if j < 4:                                     # a unit vector's commitment IS the column: the words themselves
                assert (ca == host[:, (0, n - 1, n // 2 - 1, n // 2)[j]]).all()
        assert a.generate_matrix(seed, kappa, n, iters=2) > 0 and (a.commit(vecs[4]) == b.commit(vecs[4])).all()
        a.set_witness(vecs[4])
        with pytest.raises(plus.LfPlusError) as e:        # the matrix comes before the witness
            a.generate_matrix(seed, kappa, n)
        assert e.value.code == plus.E_ARG
    finally:
        a.close()
        b.close()
