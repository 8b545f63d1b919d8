"""Goldilocks, b = 2: one fold step of two DIFFERENT witnesses under every switch set of tests/fold_paths.py, word for word against the CPU oracle's step for
exactly that pair (tests/two_sided.py): the proof per section, the folded LCCCS, and f, f_coeff and w_ccs of the folded witness.  After every step the path
masks the set records must be the ones the context reports, so a switch that did not take does not count as coverage.

The one-witness tests hand the same handle to both sides, so a kernel that reads the left planes for both, swaps the sides, or pairs one side's data with the
other's challenge powers passes them; tests/test_two_sided_cpu.py shows that the oracle's step differs in every round message for these pairs when that happens.

Shapes: T10 (m = N = 1024: GEMM rounds 1..3 all have at least 64 pairs and mode 7 runs) with every pair; G5 (N = 320 of 512 rows, L 5, K 15), E22, R61 (ragged
N = 244, n = 63: the int8 dot declines) and SV10W (the witness shorter than the tables) with (base, chain1) and its swap.  `pytest -m gpu`."""
import numpy as np
import pytest

import fold_paths
import lfo
import two_sided
from latticefold_amd.workload import P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _devices():
    yield
    two_sided.close_devices()


@pytest.mark.parametrize("case", two_sided.GOLD_CASES, ids=two_sided.case_id)
def test_every_switch_set_folds_two_witnesses_like_the_oracle(case, monkeypatch):
    ring, name, ccs, K, mode, pair = case
    c = two_sided.case(ring, name, pair, ccs, K, mode)
    two_sided.run_sets(c, fold_paths.GOLD_SETS, monkeypatch, fold_paths.expected, fold_paths.applied)


@pytest.mark.parametrize("pair", two_sided.SWAP, ids=lambda p: "+".join(p))
def test_generic_nonresidue_kernels_fold_two_witnesses_like_the_oracle(pair, monkeypatch):
    """F_{p^3} = F_p[Y]/(Y^3 - w^5), w = 2^40, as test_gpu_parity.py::test_fold_step_with_another_nonresidue sets it: every round kernel runs in its generic-nu
    instantiation (mode 3 for round 3, modes 4 and 1 behind it; no product-free tables, no split form).  T8, the oracle under the same tables"""
    w = 1 << 40
    nu2 = pow(w, 5, P)
    y2 = np.zeros((8, 3), dtype=np.uint64)
    for k, e in enumerate([1, 5, 7, 11, 13, 17, 19, 23]):
        g = 1 if e % 3 == 2 else 2                   # (c Y^g)^3 = c^3 nu^g = w^e  needs  3 | e - 5 g
        assert (e - 5 * g) % 3 == 0
        y2[k, g] = pow(w, ((e - 5 * g) % 24) // 3, P)
    nr, y = lfo.get_ring()
    dev = None
    try:
        assert lfo.set_ring(nu2, y2) == 0
        key = two_sided.shape_key(two_sided.G, "T8")
        dev = two_sided.DeviceShape(key, sh=two_sided.OracleShape(key), ring_tables=(nu2, y2.reshape(-1)))
        c = two_sided.case_of(dev, pair)
        sets = [ps for ps in fold_paths.GOLD_SETS if ps.name in ("default", "fused fix", "unfused, theta / u evaluated") or ps.name.startswith("lut + tab")]
        assert len(sets) == 9
        # (the product-free tables and the split form belong to the 2^40 non-residue: no GEMM round without its switch, no split round at all)
        two_sided.run_sets(c, sets, monkeypatch, lambda ps, wl: (0, 0), fold_paths.applied)
    finally:
        if dev:
            dev.close()
        assert lfo.set_ring(nr, y) == 0
