"""The wide CCS envelope (t <= 8, d <= 7) on sharded Goldilocks contexts: a fold step sharded over 2, 4 and 8 ranks must return, on EVERY rank, the words of the
unsharded run on the same device, which tests/test_gpu_wide_ccs.py pins to the oracle (one case here is compared with the live oracle as well).  Ranks share
cuda:0 and exchange through gloo, as in tests/test_dist_shard.py.  Every sharded case needs lf_ccs_load to accept t > 4 or d > 3 on a sharded context."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu
UNSUPPORTED = -3

WORKER = textwrap.dedent('''
    import os, sys, json, hashlib
    sys.path.insert(0, os.environ["LF_ROOT"]); sys.path.insert(0, os.path.join(os.environ["LF_ROOT"], "tests"))
    import numpy as np, torch.distributed as dist
    from latticefold_amd import api, dist as lfd
    import test_gpu_wide_ccs as wide              # general_deg5 / three_products: the two shapes make_workload has no kind for
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    out = {}
    for name in os.environ["LF_CASES"].split(","):
        wl = wide._wl(*name.split("/"))
        def run(sharded):
            ctx = api.Context(0)
            tr = lambda: api.PoseidonTranscript()
            if sharded:
                lfd.init_sharding(ctx, rank, world, "host")
            ctx.load_ccs(wl)
            scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
            wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
            cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
            acc, lin = api.LFLinearizationProver.prove(ctx, cccs, wit, tr())
            lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr())
            lc2, w1, proof2 = api.NIFSProver.prove(ctx, lc, w0, cccs, wit, tr())   # chained step
            h = hashlib.sha256()
            for a in (cccs, acc, lc, proof, w0.f_coeff, lc2, proof2, w1.f_coeff):
                h.update(np.ascontiguousarray(a).tobytes())
            paths = ctx.fold_paths()
            step = (wit, cccs, acc, lin, lc, w0, proof)
            bad = None
            if sharded and rank == 0 and os.environ.get("LF_ORACLE"):   # rank 0's sharded step against a live oracle step, section by section
                try:
                    wide._assert_step_equal(wl, step, wide._oracle_step(wl))
                    bad = ""
                except AssertionError as e:
                    bad = str(e) or "differs"
            ctx.close()
            return h.hexdigest() + ":%d" % paths, bad
        ref = run(False)[0] if rank == 0 else None
        got, bad = run(True)
        allg = [None] * world
        dist.all_gather_object(allg, got)
        if rank == 0:
            out[name] = {"ref": ref, "ranks": allg, "oracle": bad}
    if rank == 0:
        print(json.dumps(out))
    dist.destroy_process_group()
''')

BIG = dict(LF_FOLD_LUT_MIN="128", LF_FOLD_FUSE_MIN="64", LF_FOLD_TAB_MIN="64")
ENVS = {
    None: {},
    "deep": dict(BIG, LF_SHARD_LIN_MIN="0", LF_SHARD_FOLD_MIN="0"),                 # the latest hand-over: only the 64-pairs-per-rank rule
    "early": dict(BIG, LF_SHARD_LIN_MIN="1048576", LF_SHARD_FOLD_MIN="1048576"),    # the earliest: gathered after the first fix
    "gemm": dict(BIG, LF_FOLD_SV_MIN="64", LF_DOT_MIN="64"),                        # (LF_DOT_MIN: the int8 inner products on the ranks' column slices, odd first columns included)
    "one": dict(LF_SHARD_TWO_LANES="0"),                                            # one host thread issues every exchange
}


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run_worker(tmp_path, world, cases, mode, oracle=False):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, LF_ROOT=ROOT, OMP_NUM_THREADS="2", LF_CASES=cases)
    env.update(ENVS[mode])
    if oracle:
        env["LF_ORACLE"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


# the smallest shapes that reach each branch:
#   world 2, T10: NP = 6 and 9 and a non-unit c_i (mix8); the hand-over falls in round 3 by the 64-pairs-per-rank rule
#   world 4, T12 mix8 / general5: two-entry rows that refer to a neighbour's and, wrapping round, to rank 0's columns -- shard_col_range over six matrices,
#            k_spmv_rows in chunks on sliced rows
#   world 2, T10/three6: t = 6 at d = 2, the NP = 5 instantiation
#   world 4, T14/deg5 deep / early: the latest and the earliest hand-over
#   world 8, T14/deg7 gemm: the int8 inner products on column slices at t = 8, in groups of two
#   world 2, T12/deg5 one: the one-channel schedule
@pytest.mark.parametrize("world,cases,mode", [(2, "T10/deg4,T10/deg7,T10/mix8", None), (4, "T12/mix8,T12/general5", None), (2, "T10/three6", None),
                                              (4, "T14/deg5", "deep"), (4, "T14/deg5", "early"), (8, "T14/deg7", "gemm"), (2, "T12/deg5", "one")])
def test_sharded_wide_fold_step_equals_unsharded(tmp_path, world, cases, mode):
    d = _run_worker(tmp_path, world, cases, mode)
    assert sorted(d) == sorted(cases.split(","))
    for name, r in d.items():
        assert len(r["ranks"]) == world
        assert all(x.split(":")[0] == r["ref"].split(":")[0] for x in r["ranks"]), (name, r)
        if mode == "gemm":   # every rank and the unsharded reference ran rounds 1-3 as GEMMs (fold_paths mask behind the digest)
            assert r["ref"].endswith(":7") and all(x.endswith(":7") for x in r["ranks"]), r


def test_sharded_wide_fold_step_equals_the_live_oracle(tmp_path):
    """world 2, T10/deg7: rank 0's lf_linearize proof and every section of its fold proof against a live lfo.Instance step, not only the unsharded device run"""
    d = _run_worker(tmp_path, 2, "T10/deg7", None, oracle=True)
    r = d["T10/deg7"]
    assert r["oracle"] == "", r["oracle"]
    assert all(x.split(":")[0] == r["ref"].split(":")[0] for x in r["ranks"]), r


def _model_step(wl, rank, world):
    """rank `rank` of `world` with the model transport: the exchange count and the words of one fold step"""
    from latticefold_amd import api
    ctx = api.Context(0)
    try:
        ctx.set_sharding_model(rank, world)
        ctx.load_ccs(wl)
        scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        tr = api.PoseidonTranscript()
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr)
        ctx.dist_stats(reset=True); ctx.dist_stats_words(reset=True)
        api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr)
        return ctx.dist_stats()[0], ctx.dist_stats_words()
    finally:
        ctx.close()


def test_model_transport_runs_a_wide_ranks_share():
    """lf_set_sharding_model and a wide lf_ccs_load: the step runs to completion, and a rank issues as many exchanges as the same rank of the R1CS step of that
    size -- u_s and eta of all t matrices travel in the exchanges that carry them at t = 3"""
    from latticefold_amd.workload import make_workload
    wide, r1cs = make_workload("T14", 0, ccs="deg7"), make_workload("T14")
    assert (wide.t, wide.d, r1cs.t) == (8, 7, 3)
    assert _model_step(wide, 0, 1) == (0, 0)
    for G, r in ((2, 1), (4, 0), (4, 3)):
        n_w, words_w = _model_step(wide, r, G)
        n_r, words_r = _model_step(r1cs, r, G)
        assert n_w == n_r > 8, (G, r, n_w, n_r)
        assert words_w > words_r > 0, (G, r, words_w, words_r)   # (more tables in the hand-over, longer round messages)


def _load_rc(ctx, wl):
    from latticefold_amd import api
    try:
        ctx.load_ccs(wl)
    except api.LfError as e:
        return e.code
    return 0


def test_refusals_that_stay_leave_the_context_usable():
    import test_gpu_wide_ccs as wide
    from latticefold_amd import api
    from latticefold_amd.workload import make_workload
    w8 = wide._wl("T8", "deg7")
    w8.d = 8                                                      # (t stays 8: the degree alone is claimed, as in test_gpu_wide_ccs)
    for bad in (w8, make_workload("T8b4", 0, ccs="deg5")):        # d = 8; b = 4 on a sharded context
        ctx = api.Context(0)
        try:
            ctx.set_sharding_model(1, 2)
            assert _load_rc(ctx, bad) == UNSUPPORTED
            ctx.set_sharding_model(0, 1)                          # (the oracle comparison below needs the whole step: back to the plain context)
            wl = make_workload("T8", 0)
            ctx.load_ccs(wl)
            case = wide.Case.__new__(wide.Case)
            case.wl, case.ctx = wl, ctx
            case.scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
            wide._assert_step_equal(wl, wide._gpu_step(case), wide._oracle_step(wl))
        finally:
            ctx.close()


def test_babybear_refuses_a_wide_ccs_and_stays_usable():
    import lfo_bb
    from latticefold_amd import api
    from latticefold_amd.workload import make_workload
    ctx = api.Context(0, ring="babybear")
    try:
        assert _load_rc(ctx, make_workload("B6", 0, ccs="deg4")) == UNSUPPORTED
        wl = make_workload("B6", 0)
        ctx.load_ccs(wl)
        A = wl.ajtai_matrix()
        scheme = api.AjtaiCommitmentScheme(ctx, matrix=A)
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        tr = lambda: api.PoseidonTranscript(ring="babybear")
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr())
        lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr())
        inst = lfo_bb.Instance(wl)
        f = inst.witness_from_w_ccs(wl.w_ccs)
        acc_o, _ = inst.linearize(lfo_bb.Transcript(), cccs, f)
        lc_o, f0_o, proof_o = inst.fold_step(lfo_bb.Transcript(), A, acc_o, f, cccs, f)
        assert (acc == acc_o).all() and (proof == proof_o).all() and (lc == lc_o).all() and (w0.f == f0_o).all()
    finally:
        ctx.close()
