"""Rounds 1..3 of the folding sumcheck as int8 GEMMs (lf_sv_rounds.hip: k_sv_gemm) at the shapes where its K loop can go wrong: whole fold steps
through the C ABI against the CPU oracle, as tests/test_gpu_parity.py::test_fold_step_gemm_rounds_match_oracle runs them (LF_FOLD_SV_MIN = LF_DOT_MIN = 64,
LF_FOLD_SV_ROUNDS 1 / 2 / 3), in the split form (one eq value per pair: two column tiles) and with LF_FOLD_SV_NO_SPLIT=1 (three column tiles; V = 4 then has
six pair groups instead of four).  Proof, folded LCCCS and f_0 must equal the oracle's word for word."""
import numpy as np
import pytest

import fold_paths
import lfo
import test_gpu_bb as bb
from latticefold_amd import api, workload
from latticefold_amd.workload import make_workload
from test_gpu_parity import run_both

pytestmark = pytest.mark.gpu

# name: (s, wit_len, L, B, b, K, kappa) -- entries of this file only
SHAPES = {
    # the smallest legal round (sv_shape_ok: 64 pairs) is round 1 of SV7 and round 3 of SV9: a chunk is ONE super-step, the loop's first iteration is its last
    # (it prefetches its own index), and at V = 1 that super-step is a quarter full (64 of 256 pairs; the rest are zero words of the padded bit planes)
    "SV7": (7, 32, 4, 1 << 16, 2, 16, 4),
    "SV9": (9, 128, 4, 1 << 16, 2, 16, 4),
    # a witness shorter than the tables (N = 800 of 1024 rows): the pairs behind ceil(N / 2V) are not visited, and the last super-step is partly zero words
    "SV10W": (10, 200, 4, 1 << 16, 2, 16, 4),
    # unequal chunks (see test_unequal_chunks_shape): 11 super-steps, two tiles of digit planes (K = 17); N = 5600 of 8192 rows
    "SV13U": (13, 1400, 4, 1 << 17, 2, 17, 2),
    "SV10X": (10, 256, 4, 1 << 16, 2, 16, 4),      # base of the digit-extreme witnesses
}


@pytest.fixture(scope="module", autouse=True)
def _shapes():
    workload.CONFIGS.update(SHAPES)
    yield
    for k in SHAPES:
        workload.CONFIGS.pop(k, None)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bb_ctx():
    c = api.Context(0, ring=bb.RING)
    yield c
    c.close()


def sv_chunks(V, nsuper, K, rd=24):
    """mirror of sv_chunks_n (lf_sv_rounds.hip): (chunks, super-steps per chunk) of a round's GEMM launches"""
    per_chunk = rd * 2 * ((K + 15) // 16) // (8 if V <= 2 else 4)
    want = max(1, min(256 // per_chunk, nsuper))
    spc = -(-nsuper // want)
    return -(-nsuper // spc), spc


def gemm_rounds(ctx, monkeypatch, wl, acc_g, wit, cccs, ref, forms=fold_paths.SV_FORMS, transcript=api.PoseidonTranscript, dot_min=True):
    lc_o, f0_o, proof_o = ref
    for k, v in dict(fold_paths.SV_MIN, **(fold_paths.SV_DOT_MIN if dot_min else {})).items():
        monkeypatch.setenv(k, v)
    m = 1 << wl.s
    for rounds in fold_paths.SV_ROUNDS:
        monkeypatch.setenv("LF_FOLD_SV_ROUNDS", str(rounds))
        for extra in forms:
            for k, v in extra.items():
                monkeypatch.setenv(k, v)
            lc, w, proof = api.NIFSProver.prove(ctx, acc_g, wit, cccs, wit, transcript())
            for k in extra:
                monkeypatch.delenv(k)
            want = sum(1 << (r - 1) for r in range(1, rounds + 1) if (m >> r) >= 64)
            assert ctx.fold_paths() == want, (rounds, extra, ctx.fold_paths(), want)      # the rounds really ran as GEMMs
            bad = np.nonzero((proof != proof_o).any(axis=1))[0]
            assert bad.size == 0 and (lc == lc_o).all() and (w.f == f0_o).all(), (rounds, extra, bad[:6])


def test_unequal_chunks_shape():
    """SV13U really has a shorter last chunk in round 3 (V = 4): 11 super-steps in chunks of 2.  For V <= 2 the chunk count reaches the number of
    super-steps up to 21 (K >= 17) or 42 (K = 16) of them, i.e. unequal chunks first appear at 2^14 rows, where the oracle's fold step takes longer than a
    test of this suite may; the clamp of a chunk's end and the prefetch index are the same lines of k_sv_gemm for every V."""
    s, wit_len, L, _B, _b, K, _kappa = SHAPES["SV13U"]
    nsuper = -(-wit_len * L // 512)
    assert wit_len * L < (1 << s) and nsuper == 11
    chunks, spc = sv_chunks(4, nsuper, K)
    assert (chunks, spc) == (6, 2) and nsuper % spc != 0
    assert sv_chunks(1, nsuper, K) == (11, 1) and sv_chunks(2, nsuper, K) == (11, 1)


@pytest.mark.parametrize("name", ["SV7", "SV9", "SV10W", "SV13U"])
def test_gemm_rounds_edge_shapes(ctx, name, monkeypatch):
    wl, inst, A, f_coeff, wit, cccs, acc_g, _, acc_o, _ = run_both(ctx, name, 2)
    ref = inst.fold_step(lfo.Transcript(), A, acc_o, f_coeff, cccs, f_coeff)
    gemm_rounds(ctx, monkeypatch, wl, acc_g, wit, cccs, ref)


@pytest.mark.parametrize("kind", ["zero", "max", "min"])
def test_gemm_rounds_digit_extremes(ctx, kind, monkeypatch):
    """every coefficient of the witness 0, +(B/2 - 1) or -(B/2 - 1) in every digit: all bit planes zero, or the 15 magnitude planes all ones with the sign
    planes all clear / all set -- every monomial's AND and sign product take their extreme value in every byte of every operand, and the int32 tiles reach
    the largest sums of the shape (512 / 256 / 128 pairs of +-1 times a digit of at most 128 in magnitude)"""
    wl = make_workload("SV10X", 2)
    h = wl.B // 2 - 1
    value = sum(h * wl.B ** i for i in range(wl.L))
    assert value < api.P
    coeff = np.full((wl.wit_len, 24), {"zero": 0, "max": value, "min": api.P - value}[kind], dtype=np.uint64)
    wl.w_ccs = lfo.crt(coeff)
    wl.val[2] = np.ascontiguousarray(wl.z()[:min(wl.n, wl.m)])     # C = diag(z) of this witness: the CCS stays satisfied
    inst = lfo.Instance(wl)
    ctx.load_ccs(wl)
    A = wl.ajtai_matrix()
    scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
    f_coeff = inst.witness_from_w_ccs(wl.w_ccs)
    assert (f_coeff == np.uint64({"zero": 0, "max": h, "min": api.P - h}[kind])).all()
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    assert (wit.f_coeff == f_coeff).all()
    cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
    acc_g, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
    acc_o, _ = inst.linearize(lfo.Transcript(), cccs, f_coeff)
    assert (acc_g == acc_o).all()
    ref = inst.fold_step(lfo.Transcript(), A, acc_o, f_coeff, cccs, f_coeff)
    gemm_rounds(ctx, monkeypatch, wl, acc_g, wit, cccs, ref)


def test_gemm_rounds_babybear_smallest(bb_ctx, monkeypatch):
    """BabyBear (72 coefficient groups per side: 18 blocks of 8 groups per chunk instead of 6) at its smallest GEMM round: round 1 of BDP, 64 pairs"""
    wl, inst, A, f_coeff, wit, cccs, acc_g, _, acc_o, _ = bb.run_both(bb_ctx, "BDP", 2)
    assert (1 << wl.s) >> 1 == 64
    ref = inst.fold_step(bb.lfo.Transcript(), A, acc_o, f_coeff, cccs, f_coeff)
    gemm_rounds(bb_ctx, monkeypatch, wl, acc_g, wit, cccs, ref, forms=({},), transcript=bb.tr_new, dot_min=False)
