"""The real bench.py on one GPU, one process: the plain line (no --full) and --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """a plain run (no --full) prints the headline without the reporting extras; --dump-outputs writes the last timed step's outputs as float32 bytes of
    the uint64 words, identical in two runs with the same arguments, and the dumped proof is the one the oracle-only fixture of the workload names"""
    import hashlib
    import numpy as np
    lines = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--workload", "B14", "--dump-outputs", str(tmp_path / run)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-6
    for k in ("roofline", "ajtai", "ivc", "shard_model", "lfplus", "cpu_baseline"):
        assert k not in d, k
    assert "matches_oracle_fixture" not in d["config"]
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == sorted(n + ".npy" for n in ("lcccs", "proof", "folded_witness_f", "folded_witness_f_coeff", "folded_witness_w_ccs")), names
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.shape[-1] == 8 and (a == b).all(), n
    words = lambda n: np.load(tmp_path / "a" / n).astype(np.uint8).reshape(-1, 8).copy().view("<u8").reshape(-1)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "scale_digests.json")))["B14"]
    assert hashlib.sha256(words("proof.npy").tobytes()).hexdigest() == gold["proof"]
    assert hashlib.sha256(words("lcccs.npy").tobytes()).hexdigest() == gold["lcccs_out"]
