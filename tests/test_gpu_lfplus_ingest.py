"""Instance ingestion of the LatticeFold+ slice on the GPU: lfplus_witness_from_z (ComR1CS::new, crates/latticefold-plus/src/r1cs.rs:48-60: f =
z.gadget_decompose(b, k) cut and committed on the device, only z uploaded), lfplus_commit_resident, ComR1CS.new_resident and PlusProver.ingest -- word for
word against the oracle (oracle/lfp.c through tests/lfp.py), the committed oracle-only digests, and the upload path it replaces.  Bit-exact: no tolerance."""
import hashlib
import json
import os
from math import ceil, log, sqrt

import numpy as np
import pytest

import lfp
from latticefold_amd import plus
from test_lfplus_ingest_cpu import edge_z

pytestmark = pytest.mark.gpu
D, P = 16, plus.P
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lfplus_digests.json")
CM_KEYS = ("msgs", "r", "e", "b", "v", "a", "bb", "c", "comh", "pa", "ea", "pb", "eb", "ro", "cm_g", "vo", "fcoms")

# (kappa, k, b, n): kappa in {1, 2, 5} (launch groups 1, 2, 4 + 1), every k and b of the envelope's list, n from 2^6 to 2^15.  The kernel's tile is 16 elements
# of z (16 k rows of f), a block takes whole tiles: (1, 16, 2, 64) and (5, 4, 3108, 64) have fewer rows than one tile, (1, 4, 16, 400) and (2, 3, 7, 111) end
# inside a tile, 2^15 rows with k = 1 is 2048 blocks
CASES = [
    (1, 1, 2, 1 << 6), (1, 16, 2, 1 << 6), (5, 4, 3108, 1 << 6), (5, 1, 3, 1 << 6), (2, 4, 3, 1 << 7), (2, 1, 1 << 31, 1 << 8), (5, 2, 8, 1 << 9),
    (2, 4, 3109, 1 << 10), (2, 16, 1 << 31, 1 << 10), (1, 2, 1 << 20, 1 << 11), (2, 4, 3108, 1 << 12), (1, 16, 16, 1 << 13), (5, 4, 16, 1 << 14),
    (1, 4, 8, 1 << 15), (2, 1, 3108, 1 << 15), (5, 2, 1 << 20, 1 << 15), (1, 4, 16, 400), (2, 3, 7, 111),
]


def _patterns(b, k, m, seed):
    rng = np.random.default_rng(seed)
    binary = np.zeros((m, D), dtype=np.uint64)
    binary[:, 0] = rng.integers(0, 2, size=m)
    return {"random": rng.integers(0, P, size=(m, D), dtype=np.uint64), "binary": binary, "edge": edge_z(b, k, m, seed)}


@pytest.mark.parametrize("kappa,k,b,n", CASES)
def test_witness_from_z_matches_the_oracle(kappa, k, b, n):
    m = n // k
    A = lfp.splitmix(40 + kappa, 0, kappa * n * D).reshape(kappa, n, D)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        for name, z in _patterns(b, k, m, n + k).items():
            cm = ctx.witness_from_z(z, b, k)
            f = ctx.get_witness()
            slow = name == "random" and n >= 1 << 12          # (the oracle binding builds a table per distinct value)
            want = plus.gadget_decompose(z, b, k) if slow else lfp.gadget_decompose(z, b, k)
            assert f.shape == want.shape and (f == want).all(), (name, "f")
            assert (cm == lfp.commit(A, want)).all(), (name, "cm_f")
            assert (ctx.commit_resident() == cm).all(), (name, "commit_resident")
            assert (ctx.commit(f) == cm).all(), (name, "commit")
            assert (ctx.get_witness() == want).all(), (name, "the witness is still resident after the commits")
    finally:
        ctx.close()


def _rg_read(ctx, dp):
    ctx._chk(plus._lib().lfplus_rg_from_f(ctx.h, dp.b, dp.k, dp.l))
    k, n, kappa = dp.k, ctx.n, ctx.kappa
    Df, com = np.zeros((k, n, D), dtype=np.int8), np.zeros((k, kappa, D, D), dtype=np.uint64)
    tau, mt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int8)
    c = [np.zeros((kappa, D), dtype=np.uint64) for _ in range(3)]
    ctx._chk(plus._lib().lfplus_rg_read(ctx.h, Df.ctypes.data_as(plus.i8p), com.ctypes.data_as(plus.u64p), tau.ctypes.data_as(plus.u64p), mt.ctypes.data_as(plus.i8p),
                                        *[x.ctypes.data_as(plus.u64p) for x in c]))
    return [Df, com, tau, mt] + c


def test_from_f_sees_the_ingested_witness_also_behind_a_pending_async_pass():
    wl = plus.make_plus_workload("P15")
    dp, A = wl.params().lin.decomp, wl.ajtai_matrix()
    z0, z1 = wl.z(0), wl.z(1)
    f0, f1 = plus.gadget_decompose(z0, wl.B, wl.k), plus.gadget_decompose(z1, wl.B, wl.k)
    ctx = plus.PlusContext(0)
    try:
        ctx.set_matrix(A)
        ctx.set_witness(f0)
        want0 = _rg_read(ctx, dp)
        ctx.set_witness(f1)
        want1 = _rg_read(ctx, dp)
        assert not all((a == b).all() for a, b in zip(want0, want1))
        cm = ctx.witness_from_z(z0, wl.B, wl.k)
        got = _rg_read(ctx, dp)
        assert all((a == b).all() for a, b in zip(got, want0)) and (cm == want0[4]).all()
        ctx.rg_from_f_async(dp)                      # a pass over f0 in flight ...
        cm = ctx.witness_from_z(z1, wl.B, wl.k)      # ... must be joined before f1 overwrites the witness it reads
        got = _rg_read(ctx, dp)
        assert all((a == b).all() for a, b in zip(got, want1)) and (cm == want1[4]).all()
        ctx.rg_from_f_async(dp)
        assert (ctx.commit_resident() == want1[4]).all()
        got = _rg_read(ctx, dp)
        assert all((a == b).all() for a, b in zip(got, want1))
    finally:
        ctx.close()


def _no_uploads(monkeypatch, prover, fresh):
    """PlusContext.set_witness / commit raise for the contexts of the fresh instances: the ingest path must not fall back to an upload of f"""
    banned = {id(c) for c in fresh}
    real_set, real_commit = plus.PlusContext.set_witness, plus.PlusContext.commit

    def set_witness(self, f):
        assert id(self) not in banned, "set_witness on a fresh instance's context"
        return real_set(self, f)

    def commit(self, v):
        assert id(self) not in banned, "commit (upload of f) on a fresh instance's context"
        return real_commit(self, v)
    monkeypatch.setattr(plus.PlusContext, "set_witness", set_witness)
    monkeypatch.setattr(plus.PlusContext, "commit", commit)


def _bound(L, k):
    a, c = 16 * 128 * L, 8 + 16 * k + 1                  # utils::estimate_bound (utils.rs:102-112)
    return ceil((a + sqrt(a * a + 4 * a * c)) / 2)


def _same(got, want, keys, where):
    for key in keys:
        assert (np.asarray(got[key]) == np.asarray(want[key])).all(), (where, key)


def test_ingested_proves_match_the_live_oracle(monkeypatch):
    """the accumulating shape of tests/test_gpu_lfplus_prover.py::test_plus_prover_matches_oracle (kappa 1, k 4, rounds (2, 1, 1), device_acc), every instance
    built by PlusProver.ingest"""
    n, L, kappa, k, rounds = 1 << 15, 3, 1, 4, (2, 1, 1)
    B = _bound(L, k) // 2
    l = ceil(log(P) / log(8))
    A = lfp.splitmix(23, 0, kappa * n * D).reshape(kappa, n, D)
    r1cs = plus.r1cs_decomposed_square((plus.identity_csr(n // k),) * 3, n, B, k)
    params = plus.PlusParameters(plus.LinParameters(kappa, plus.DecompParameters(8, k, l)), B)
    rng = np.random.default_rng(8)
    zs_all = []
    for ncomp in rounds:
        zs = []
        for _ in range(ncomp):
            z = np.zeros((n // k, D), dtype=np.uint64)
            z[:, 0] = rng.integers(0, 2, size=n // k)
            zs.append(z)
        zs_all.append(zs)
    oracle = lfp.PlusOracle(A, list(r1cs), kappa, 8, k, l, B, lfp.Transcript())
    prover = plus.PlusProver.init(A, list(r1cs), 1, params, plus.PoseidonTranscript())
    prover.device_acc = True
    ver, ts_o = plus.PlusVerifier.init(A, list(r1cs), params, plus.PoseidonTranscript()), lfp.Transcript()
    try:
        for zs in zs_all:
            want = oracle.prove([(lfp.gadget_decompose(z, B, k), r1cs) for z in zs])
            nacc = len(prover.acc)
            _no_uploads(monkeypatch, prover, prover.ctxs[nacc:nacc + len(zs)])
            comps = prover.ingest(zs, r1cs)
            assert all(ci.f is None and ci.ctx is prover.ctxs[nacc + i] for i, ci in enumerate(comps))
            got = prover.prove(comps)
            monkeypatch.undo()
            for i in range(len(zs)):
                _same(got["lproof"][i], want["lproof"][i], ("msgs", "r", "evals"), f"lproof[{i}]")
            _same(got["cmproof"], want["cmproof"], CM_KEYS, "cmproof")
            _same(got["linb2x"], want["linb2x"], ("cm_g", "ro", "vo"), "linb2x")
            _same(got["dproof"], want["dproof"], ("C0", "C1", "v0", "v1"), "dproof")
            acc = prover.accumulator()
            for i in range(2):
                assert (acc[i] == oracle.acc[i]).all()
            assert ver.verify(got), ver.stage
            assert lfp.plus_verify(ts_o, got, B) == 0
        assert prover.transcript.get_challenge() == oracle.tr.challenge()
    finally:
        prover.close()
        plus.scratch_trim(0)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def digests(proof, acc, challenge):
    """as tests/test_gpu_lfplus_scale.py::digests (the layout of tests/golden/lfplus_digests.json)"""
    d = {"final_challenge": int(challenge), "acc_F0": _sha(acc[0]), "acc_F1": _sha(acc[1])}
    for i, lp in enumerate(proof["lproof"]):
        for key in ("msgs", "r", "evals"):
            d[f"lproof{i}_{key}"] = _sha(lp[key])
    for key in CM_KEYS:
        d[f"cm_{key}"] = _sha(proof["cmproof"][key])
    for key in ("cm_g", "ro", "vo"):
        d[f"linb2x_{key}"] = _sha(proof["linb2x"][key])
    for key in ("C0", "C1", "v0", "v1"):
        d[f"dproof_{key}"] = _sha(proof["dproof"][key])
    return d


@pytest.mark.parametrize("name", ["P15", "P16", "P17", "P20"])
def test_ingested_prove_matches_committed_oracle_digests(name, monkeypatch):
    want = {k: v for k, v in json.load(open(GOLD))[name].items() if k not in ("oracle_seconds", "oracle_host", "workload", "first_words")}
    wl = plus.make_plus_workload(name)
    A, r1cs = wl.ajtai_matrix(), wl.r1cs()
    prover = plus.PlusProver.init(A, list(r1cs), max(1, wl.L - 2), wl.params(), plus.PoseidonTranscript(), 0)
    try:
        _no_uploads(monkeypatch, prover, prover.ctxs[:wl.L])
        comps = prover.ingest([wl.z(i) for i in range(wl.L)], r1cs)
        proof = prover.prove(comps)
        monkeypatch.undo()
        got = digests(proof, prover.acc, prover.transcript.get_challenge())
    finally:
        prover.close()
    bad = [k for k in want if got.get(k) != want[k]]
    assert not bad, f"{name}: fields differing from the oracle fixture: {bad}"
    ver = plus.PlusVerifier.init(A, list(r1cs), wl.params(), plus.PoseidonTranscript())
    assert ver.verify(proof), ver.stage


def _refused(ctx, z, b, k):
    with pytest.raises(plus.LfPlusError) as e:
        ctx.witness_from_z(z, b, k)
    assert e.value.code == plus.E_ARG, e.value
    for call in (ctx.get_witness, ctx.commit_resident, lambda: ctx._chk(plus._lib().lfplus_rg_from_f(ctx.h, 8, 4, 22))):
        with pytest.raises(plus.LfPlusError) as e2:      # no resident witness after a refusal
            call()
        assert e2.value.code == plus.E_ARG
    return str(e.value)


def test_refusals_leave_no_witness_and_the_context_usable():
    wl = plus.make_plus_workload("P15")
    n, k, B = wl.n, wl.k, wl.B
    A, z = wl.ajtai_matrix(), wl.z(0)
    f = plus.gadget_decompose(z, B, k)
    ctx, bare, sharded = plus.PlusContext(0), plus.PlusContext(0), plus.PlusContext(0)
    try:
        bare.n = n
        assert "matrix" in _refused(bare, z, B, k)
        ctx.set_matrix(A)
        for pos in ((0, 0), (n // k - 1, D - 1), (n // (2 * k) + 1, 3)):
            ctx.set_witness(f)                           # a resident witness that the refused call must not leave behind
            bad = z.copy()
            bad[pos] = np.uint64(P + (pos[1] % 2))
            assert "non-canonical" in _refused(ctx, bad, B, k)
        for zz, b, kk in ((z[:-1], B, k), (z, B, 2), (z, 1, k), (z, (1 << 31) + 1, k), (z, B, 0), (np.zeros((n // 17 + 1, D), dtype=np.uint64), B, 17)):
            ctx.set_witness(f)
            _refused(ctx, zz, b, kk)
        cm = ctx.witness_from_z(z, B, k)                 # the context works again
        assert (ctx.get_witness() == f).all() and (cm == lfp.commit(A, f)).all()
        sharded.set_sharding_model(0, 2)
        sharded.set_matrix(wl.ajtai_matrix((0, n // 2)))
        with pytest.raises(plus.LfPlusError) as e:
            sharded.witness_from_z(z, B, k)
        assert e.value.code == plus.E_ARG and "sharded" in str(e.value)
        sharded.set_witness(f)
        with pytest.raises(plus.LfPlusError) as e:
            sharded.commit_resident()
        assert e.value.code == plus.E_ARG and "sharded" in str(e.value)
    finally:
        for c in (ctx, bare, sharded):
            c.close()


def test_a_failed_ingest_fails_the_prover_and_foreign_resident_instances_are_refused():
    wl = plus.make_plus_workload("P15")
    A, r1cs = wl.ajtai_matrix(), wl.r1cs()
    prover = plus.PlusProver.init(A, list(r1cs), max(1, wl.L - 2), wl.params(), plus.PoseidonTranscript(), 0)
    other = plus.PlusProver.init(A, list(r1cs), max(1, wl.L - 2), wl.params(), plus.PoseidonTranscript(), 0)
    try:
        zs = [wl.z(i) for i in range(wl.L)]
        comps = other.ingest(zs, r1cs)
        assert (comps[1].fetch_f() == plus.gadget_decompose(zs[1], wl.B, wl.k)).all()
        with pytest.raises(plus.LfPlusError):
            prover.prove(comps)                          # resident in another prover's contexts
        bad = zs[1].copy()
        bad[7, 7] = np.uint64(P)
        fresh = plus.PlusProver.init(A, list(r1cs), max(1, wl.L - 2), wl.params(), plus.PoseidonTranscript(), 0)
        try:
            with pytest.raises(plus.LfPlusError):
                fresh.ingest([zs[0], bad, zs[2]], r1cs)
            assert fresh.failed is not None
            with pytest.raises(plus.LfPlusError):
                fresh.ingest(zs, r1cs)
            with pytest.raises(plus.LfPlusError):
                fresh.prove([])
        finally:
            fresh.close()
    finally:
        prover.close()
        other.close()
