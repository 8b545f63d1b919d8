"""The numeric host work inside the sumcheck rounds (lf_step_host.h: eq_weights, eq_prefix, fold_lut81, split_coef, complete_fold_split, complete_lin_split)
against the definitions, for the Goldilocks and the BabyBear ring: a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "latticefold_amd", "csrc")


def test_step_host_selftest_program_under_sanitizers():
    """make step-host-selftest, fixed seed, both rings: the completed fold message (degree 4) equals g(X) = c eq(beta_i, X) (A0 + A1 X + A2 X^2 + A3 X^3) + G(X)
    at X = 0..4 in all eight slots; the completed linearization message equals c eq(beta_i, X) T(X) for every dT = 1..7; a zero c or a zero beta_i says
    "do not split"; eq_weights equals the product definition for nbits = 0..3; fold_lut81 holds sum_b (t_b - 1) W_b for the 81 codes and then the squares
    (nothing is loaded into this interpreter)"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "step-host-selftest"])
    r = subprocess.run([os.path.join(CSRC, "build", "lf_step_host_selftest")], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "step host selftest ok" in out and "MISMATCH" not in out and "runtime error" not in out and "Sanitizer" not in out
    groups = [ln for ln in out.splitlines() if ln.rstrip().endswith(" ok") and "checks" in ln]
    assert len(groups) == 10 and all(int(re.search(r"(\d+) checks", ln).group(1)) > 0 for ln in groups)
    for ring in ("goldilocks", "babybear"):
        for what in ("fold completion", "linearization completion", "invertibility test", "eq_weights", "fold_lut81"):
            assert any(ln.startswith(ring) and what in ln for ln in groups), (ring, what)
