"""The fused q_j gather-and-pack kernel (csrc/lf_dot_i8.hip, k_q_pack_i8) on the host: a stand-alone program restates its byte placement from balanced_bytes
and kstep_col and compares it, byte for byte, with the restatement of k_dot_pack_y on the same words; and the one shape test of the int8 inner products
(lf_dot_plan.h) against DotPlan::make over a case table.  Address and undefined-behaviour sanitizers; no GPU, nothing loaded into this interpreter."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "latticefold_amd", "csrc")


def test_q_pack_selftest_program_under_sanitizers():
    """make q-pack-selftest: n = 64, 66, 130, 258 columns x t = 1, 2, 3 matrices (an empty column, corner words of balanced_bytes, the zero padding of a partial
    block, the digit rows of absent matrices left alone), then the shape test: column count, na, nb, odd ldx, alignment, lead column, overflow bound,
    LF_DOT_MIN and LF_DOT_VALU"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "q-pack-selftest"])
    r = subprocess.run([os.path.join(CSRC, "build", "lf_q_pack_selftest")], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "q pack selftest ok" in out and "MISMATCH" not in out and "runtime error" not in out and "Sanitizer" not in out
    groups = [ln for ln in out.splitlines() if ln.rstrip().endswith(" ok") and "checks" in ln]
    assert len(groups) == 13 and all(int(re.search(r"(\d+) checks", ln).group(1)) > 0 for ln in groups)
    for n in (64, 66, 130, 258):
        for t in (1, 2, 3):
            assert any(ln.startswith(f"placement n={n} t={t}:") for ln in groups), (n, t)
    assert any(ln.startswith("predicate:") for ln in groups)
