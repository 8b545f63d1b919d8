"""The three-column lazy F_{p^3} sums of lf_field.cuh (A3P, fq3_premul_2p40, fq3_mul_2p40_pre) on the host: a stand-alone program compares them with
`unsigned __int128 %`, with lh5_mac + lh5_finish and with fq3_mul_2p40 under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "latticefold_amd", "csrc")


def test_a3p_selftest_program_under_sanitizers():
    """make field-selftest-a3p: corner and random operands, sums of 1, 2, 37, 288 and 3 * 65 536 products, the all-(p-1) and all-(2^64-1) sums, and the reduced
    product with a pre-multiplied operand (nothing is loaded into this interpreter)"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "field-selftest-a3p"])
    r = subprocess.run([os.path.join(CSRC, "build", "lf_field_selftest_a3p")], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "a3p selftest ok" in out and "MISMATCH" not in out and "runtime error" not in out and "Sanitizer" not in out
    groups = [ln for ln in out.splitlines() if ln.rstrip().endswith(" ok") and "checks" in ln]
    assert len(groups) == 5 and all(int(re.search(r"(\d+) checks", ln).group(1)) > 0 for ln in groups)
    assert f"{3 * 65536} x (0xffffffffffffffff" in out and f"{3 * 65536} x (0xffffffff00000000" in out
