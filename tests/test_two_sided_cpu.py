"""The conditions that make the two-witness GPU tests (tests/test_gpu_two_sided*.py) meaningful, on the CPU oracle alone: for every (shape, pair) those tests
fold, the two witnesses differ in every coefficient row, the proof's section layout adds up, and the step is side-sensitive -- against fold_step(L, R), both
fold_step(R, L) (the sides swapped) and fold_step(L, L) (the left witness on both sides) differ in every round message, in at least nine tenths of the theta
and of the eta rows, in the folded LCCCS and in f_0.  A device that read one side's planes for both sides, or swapped them, cannot then equal the reference.

The nine tenths are counted over the rows that can differ at all.  A theta or eta row belongs to one side and one digit part k.  It is zero in every step,
whatever the challenges, when that part of that side's witness is zero: the unused top digits (|f| < B/2 leaves part K - 1 of a b = 2 witness empty; +-(B/2 - 1)
has two non-zero base-4 digits), every part of the zero witness, the top parts of the folded one.  Rows that are zero in the reference AND in the other step
are left out of the count.  One more family cannot differ: theta of the left side in fold_step(L, L) when L is max or min and N = m -- every f-hat table of
such a witness is one constant over all m rows, so it evaluates to that constant at every point; those rows are asserted EQUAL and left out.  The right side
of that step (max where the reference has min) still differs in every live row, which is what a kernel reading the left planes twice would get wrong.

Also: the path masks tests/fold_paths.py expects of a step under a switch set, against the formulas the one-witness tests assert on their own shapes."""
import numpy as np
import pytest

import fold_paths
import two_sided
from latticefold_amd.workload import make_workload

CASES = two_sided.GOLD_CASES + two_sided.BB_CASES + two_sided.SB_CASES + two_sided.WIDE_CASES + two_sided.T8_CASES


def _rows_differing(a, b):
    return (np.asarray(a) != np.asarray(b)).any(axis=1)


@pytest.mark.parametrize("case", CASES, ids=two_sided.case_id)
def test_the_pair_makes_the_step_side_sensitive(case):
    ring, name, ccs, K, mode, pair = case
    ref = two_sided.reference(ring, name, pair, ccs, K, mode)
    wl, sh = ref.wl, ref.shape
    fL, fR = ref.L.f, ref.R.f
    assert fL.shape == fR.shape == (wl.N, wl.RE)
    if "zero" in pair:
        assert not (fL if pair[0] == "zero" else fR).any() and (fR if pair[0] == "zero" else fL).any(axis=0).all()
    else:
        assert (fL != fR).any(axis=0).all(), "a coefficient row c in which the two witnesses agree everywhere"      # f_coeff[:, c] is plane c
    assert two_sided.section_rows(wl) == ref.proof.shape[0] == sh.inst.proof_len
    want = two_sided.sections(wl, ref.proof)
    assert sum(v.shape[0] for k, v in want.items() if k != "proof") == ref.proof.shape[0]
    for what, (lc, f0, proof) in (("swapped", sh.step(pair[1], pair[0])), ("left on both sides", sh.step(pair[0], pair[0]))):
        got = two_sided.sections(wl, proof)
        assert _rows_differing(got["proof_fold_msgs"], want["proof_fold_msgs"]).all(), what
        for sec in ("proof_theta", "proof_eta"):
            d = _rows_differing(got[sec], want[sec])
            live = want[sec].any(axis=1) | got[sec].any(axis=1)
            half = d.size // 2
            if what == "left on both sides" and sec == "proof_theta" and pair[0] in ("max", "min") and wl.N == wl.m:
                assert not d[:half].any()
                live[:half] = False
            assert live[half:].any(), (what, sec, "no row of the right side can differ")
            assert d[live].sum() * 10 >= 9 * live.sum(), (what, sec, int(d[live].sum()), int(live.sum()))
        assert (lc != ref.lc).any() and (f0 != ref.f0).any(), what
        assert _rows_differing(f0, ref.f0).all(), what


# ---- the expectations of fold_paths.py against the one-witness tests' own formulas -----------------------------------------------------------------------
def _dims(name):
    wl = make_workload(name, 0)
    return wl, (wl.s, wl.N, wl.m)


@pytest.mark.parametrize("name", ["T10", "G5", "E22"])
def test_masks_of_the_three_column_paths(name):
    """tests/test_gpu_fold_a3p.py"""
    wl, dims = _dims(name)
    m = wl.m
    for label, (extra, r5, split) in [("default", ({}, False, False))] + list(fold_paths.A3P_PATHS.items()):
        ps = fold_paths.PathSet(label, dict(fold_paths.A3P_BASE, **extra))
        assert ps.paths(*dims) == sum(1 << (r - 1) for r in range(1, 4) if (m >> r) >= 64), (name, label)
        want_split = 0
        if split and wl.s >= 4:
            want_split |= 0b01000
            if r5 and wl.s >= 5 and wl.N % 4 == 0:
                want_split |= 0b10000
        assert ps.split(*dims) == want_split, (name, label)


@pytest.mark.parametrize("name", ["T10", "T8", "E32", "E22", "SV10W", "R61"])
def test_masks_of_the_gemm_rounds(name, monkeypatch):
    """tests/test_gpu_parity.py::test_fold_step_gemm_rounds_match_oracle and tests/test_gpu_sv_gemm_shapes.py::gemm_rounds"""
    if name in two_sided.SHAPES:
        monkeypatch.setitem(two_sided.CONFIGS, name, two_sided.SHAPES[name])
    wl, dims = _dims(name)
    m = wl.m
    cases = list(fold_paths.GEMM_CASES) + [(r, f) for r in fold_paths.SV_ROUNDS for f in fold_paths.SV_FORMS]
    for rounds, extra in cases:
        ps = fold_paths.PathSet("", dict(fold_paths.GEMM_BASE, LF_FOLD_SV_ROUNDS=str(rounds), **extra))
        assert ps.paths(*dims) == sum(1 << (r - 1) for r in range(1, rounds + 1) if (m >> r) >= 64), (name, rounds, extra)
        if "LF_FOLD_ROUNDS_NO_SPLIT" in extra or "LF_FOLD_SPLIT_MIN" not in extra:
            assert ps.split(*dims) == 0, (name, rounds, extra)
        elif wl.s >= 5 and wl.N % 4 == 0:
            assert ps.split(*dims) == 0b11000, (name, rounds, extra)
    assert fold_paths.PathSet("", dict(fold_paths.GEMM_BASE, LF_FOLD_SV_ROUNDS="2", **fold_paths.GEMM_OFF)).paths(*dims) == 0


@pytest.mark.parametrize("name", ["B10", "B8", "BDP", "B6"])
def test_masks_of_the_babybear_steps(name):
    """tests/test_gpu_bb.py: test_fold_step_gemm_rounds_match_oracle, test_fold_step_split_table_rounds_match_oracle, STEP_READOUTS"""
    wl, dims = _dims(name)
    m = wl.m
    for rounds, extra in fold_paths.BB_GEMM_CASES:
        ps = fold_paths.PathSet("", dict(fold_paths.BB_GEMM_BASE, LF_FOLD_SV_ROUNDS=str(rounds), **extra), "babybear")
        want = sum(1 << (r - 1) for r in range(1, rounds + 1) if (m >> r) >= 64) if wl.s >= 4 and wl.N <= m and wl.N % 4 == 0 else 0
        assert ps.paths(*dims) == want, (name, rounds, extra)
    for extra, want in fold_paths.BB_SPLIT_CASES:
        ps = fold_paths.PathSet("", dict(fold_paths.BB_SPLIT_BASE, **extra), "babybear")
        if wl.s < 5 or m // 4 < 4:
            want = 0
        assert ps.split(*dims) == want, (name, extra)
    default = fold_paths.PathSet("", {}, "babybear")
    assert (default.paths(*dims), default.split(*dims)) == (0, 0)


def test_every_set_is_taken_by_some_shape_of_its_ring():
    """no set of the lists is dead weight: T10 (Goldilocks) and B8 (BabyBear) take every one of them; a shape below five variables skips mode 7"""
    _, t10 = _dims("T10")
    _, b8 = _dims("B8")
    assert [ps.name for ps in fold_paths.GOLD_SETS if not ps.takes(*t10)] == []
    assert [ps.name for ps in fold_paths.BB_SETS if not ps.takes(*b8)] == []
    assert len({ps.name for ps in fold_paths.GOLD_SETS}) == len(fold_paths.GOLD_SETS) and len({ps.name for ps in fold_paths.BB_SETS}) == len(fold_paths.BB_SETS)
    r5 = [ps for ps in fold_paths.GOLD_SETS if ps.wants == "mode7"]
    assert r5 and not any(ps.takes(4, 16, 16) for ps in r5)
    gemm = [ps for ps in fold_paths.GOLD_SETS if ps.wants == "gemm"]
    assert gemm and not any(ps.takes(10, 1022, 1024) for ps in gemm)        # N % 4 != 0: no GEMM rounds
