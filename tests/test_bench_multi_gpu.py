"""The real bench.py on its N > 1 path, 2 ranks on ONE GPU (LF_FORCE_DEVICE pins both ranks to device 0, gloo replaces RCCL
because NCCL/RCCL refuses two ranks on one device): replicas (weak) and intra-step sharding (strong); checks the JSON
contract fields the driver reads."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("mode,workload", [("replicas", "T12"), ("shard", "T14"), ("replicas", "B10"), ("shard", "B14")])
def test_bench_two_ranks_one_gpu(mode, workload):
    env = dict(os.environ, LF_FORCE_DEVICE="0", LF_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--workload", workload, "--parallelism", mode, "--no-lfplus", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == ("weak" if mode == "replicas" else "strong")
    assert "cpu_baseline" not in d                      # rank 0 at N = 1 only
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    # value is the whole-job aggregate: replicas count both ranks' steps
    per_rank = d["steps"] / (d["ms_per_step"] * d["steps"] / 1e3)
    assert abs(d["value"] - (2 if mode == "replicas" else 1) * per_rank) / d["value"] < 1e-6


def test_bench_default_for_n_gpus_is_the_sharded_config():
    """`bench.py --gpus 2` with no --parallelism runs BASELINE configs[3]'s shape: ONE fold stream sharded over the ranks
    (strong scaling), logs its exchanges and reports the replicas rate of the same GPUs as an extra key"""
    env = dict(os.environ, LF_FORCE_DEVICE="0", LF_DIST_BACKEND="gloo", LF_LFPLUS_WORKLOADS="P16")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--workload", "T14", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["scaling"] == "strong" and d["config"]["parallelism"].startswith("shard x2")
    # BASELINE configs[4] next to it: the LatticeFold+ prove sharded over the same ranks, tied to the committed oracle fixture of its workload
    run = d["lfplus"]["runs"][0]
    assert run["ms"] > 0 and run["verified"] and run["matches_oracle_fixture"] and run["exchanges"]["count"] > 20 and run["parallelism"].startswith("shard x2")
    assert d["exchanges"]["exchanges_per_step"] > 10 and d["exchanges"]["transport"] == "host"
    assert d["replicas"]["scaling"] == "weak" and d["replicas"]["value"] > 0


def test_rccl_transport_single_rank_forced_exchanges():
    """the library's own RCCL transport (lf_dist_init: dlopen'ed librccl, ncclCommInitRank, in-stream ncclAllGather on device buffers
    + k_modsum) on the one GPU this box has: a 1-rank communicator with LF_DIST_FORCE_EXCHANGE=1 runs every exchange of a sharded
    fold step; the proof must equal the unsharded one (RCCL refuses two ranks on one device, so multi-rank runs use the host
    transport in tests/test_dist_shard.py)"""
    code = """
import os, sys, json, hashlib
sys.path.insert(0, %r)
import numpy as np
import torch                      # as in bench.py: PyTorch's own librccl.so is mapped first and the library must reuse it
from latticefold_amd import api
from latticefold_amd.workload import make_workload
def run(rccl):
    wl = make_workload("T12")
    ctx = api.Context(0)
    if rccl:
        ctx.dist_init(0, 1, api.dist_unique_ids())
        os.environ["LF_DIST_FORCE_EXCHANGE"] = "1"
    ctx.load_ccs(wl)
    scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
    wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
    acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, api.PoseidonTranscript())
    lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, api.PoseidonTranscript())
    n = ctx.dist_stats()[0]
    h = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (cccs, acc, lc, proof, w0.f_coeff))).hexdigest()
    os.environ.pop("LF_DIST_FORCE_EXCHANGE", None)
    ctx.close()
    return h, n
a, _ = run(False)
b, n = run(True)
print(json.dumps({"same": a == b, "exchanges": n}))
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["same"] and d["exchanges"] >= 5, d      # (round 5: v_s and u_s share one exchange, one gather per hand-over)


def test_bench_streams_mode_single_rank():
    """opt-in throughput mode: 2 independent fold streams on one GPU from one process"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--workload", "T12", "--streams", "2",
           "--no-cpu-baseline", "--no-ajtai", "--no-lfplus", "--no-shard-model", "--chain", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 1 and "2 independent streams" in d["config"]["parallelism"]
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3 / 1e3)) / d["value"] < 1e-6


def test_bench_falls_back_to_replicas_when_the_sharded_step_fails():
    """The sharded step has never run on more than one GPU: `bench.py --gpus N` measures the replicas first and runs the sharded measurement under a watchdog;
    here rank 1's sharded measurement fails (test hook), rank 0's then never completes -- both ranks agree through the rendezvous store, rank 0 prints the
    replicas line ("weak", the reason in `note`) and both leave with exit code 0"""
    env = dict(os.environ, LF_FORCE_DEVICE="0", LF_DIST_BACKEND="gloo", LF_BENCH_FORCE_SHARD_FAIL="1", LF_SHARD_TIMEOUT="8", LF_SHARD_AGREE_TIMEOUT="60")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--workload", "T14", "--no-lfplus"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["scaling"] == "weak" and d["n_gpus"] == 2 and d["value"] > 0 and "sharded step not measured" in d["note"]
