"""BabyBear: one fold step of two DIFFERENT witnesses under every switch set tests/test_gpu_bb.py drives a step with (tests/fold_paths.py, BB_SETS), word for
word against the BabyBear build of the CPU oracle for exactly that pair: the proof per section, the folded LCCCS, f, f_coeff and w_ccs of the folded witness,
and the path masks each set records.  Shapes: BDP (its first GEMM round has 64 pairs) and B8; pairs (base, chain1), its swap, and the digit extremes on
opposite sides (max, min): every coefficient +(B/2 - 1) on the left and -(B/2 - 1) on the right, equal magnitude planes and opposite sign planes.
`pytest -m gpu`."""
import pytest

import fold_paths
import two_sided

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _devices():
    yield
    two_sided.close_devices()


@pytest.mark.parametrize("case", two_sided.BB_CASES, ids=two_sided.case_id)
def test_every_switch_set_folds_two_witnesses_like_the_oracle(case, monkeypatch):
    ring, name, ccs, K, mode, pair = case
    c = two_sided.case(ring, name, pair, ccs, K, mode)
    two_sided.run_sets(c, fold_paths.BB_SETS, monkeypatch, fold_paths.expected, fold_paths.applied)
