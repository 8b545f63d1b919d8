"""The chained NIFS prover object of the C ABI (lf_prover_*, include/lfhip_prover.h; api.NIFSChainProver) on the GPU: the committed oracle-only chain digests
(tests/golden/chain_digests.json) step by step under both commit placements and both ingest forms, word equality with the call-level sequence
(Witness::from_w_ccs + Witness::commit + NIFSProver::prove driven by hand) where no fixture exists, every proof through the host verifier, the decider, the
check of the fresh instance, resuming a chain, the state machine with every refusal, and the device-memory footprint of a chain in steady state.

The proofs of the external-basis case are compared word for word with the call-level sequence but not verified: lf_verify_host keeps the default basis
(include/lfhip.h), so there is no host verifier for them."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from latticefold_amd import api
from latticefold_amd.workload import chain_w_ccs, diag, make_workload
from test_gpu_relation_check import random_T
from test_relation_check_cpu import bad_rows, residual_host

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_digests.json")))
INLINE = api.NIFSChainProver.COMMIT_INLINE
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -3, -7
FRESH_BOUND = lambda wl: wl.B // 2 + 1      # Witness::from_w_ccs cuts balanced base-B digits: |coefficient| <= B/2, and the norm rule is max < bound


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def tr(wl):
    return api.PoseidonTranscript(ring=wl.ring)


def setup(wl, basis=None):
    ctx = api.Context(0, ring=wl.ring)
    if basis is not None:
        ctx.set_ext_basis(basis)
    ctx.load_ccs(wl)
    scheme = api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
    return ctx, scheme


def code_of(call):
    with pytest.raises(api.ChainProverError) as e:
        call()
    return e.value.code


# ---- 1, 3, 4: the oracle-only fixtures --------------------------------------------------------------------------------------------------------------------
FIXTURE_CASES = [(n, f, d, False) for n in ("T14", "C2", "B10") for f in (0, INLINE) for d in (False, True)] + [("T14", f, d, True) for f in (0, INLINE) for d in (False, True)]


@pytest.mark.parametrize("name,flags,dev_ingest,check", FIXTURE_CASES)
def test_chain_matches_the_oracle_fixture(name, flags, dev_ingest, check):
    """acc0 after init; per step the digests of cm (from cccs_out), proof, LCCCS, f (through accumulator) and the norm, a fresh transcript per step as in the
    fixture; the host verifier accepts every proof on (previous LCCCS, cccs_out) and returns the prover's LCCCS; decide is OK with bound B/2 after every step.
    Ingest j + 1 is issued straight after prove j, before anything of step j is looked at; check: it is followed by check_fresh before the prove."""
    gold = GOLD[name]
    wl = make_workload(name)
    ctx, _scheme = setup(wl)
    pr = None
    try:
        pr = api.NIFSChainProver(ctx, flags)
        acc, _ = pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
        assert sha(acc) == gold["acc0"]
        assert pr.decide() == set() and pr.steps() == 0     # (the norm bound B/2 holds for folded witnesses; a fresh one has base-B digits up to B/2 itself)
        ws = [np.ascontiguousarray(chain_w_ccs(wl, j)) for j in range(1, len(gold["steps"]) + 1)]
        wd = [dev(w) for w in ws] if dev_ingest else ws
        pr.ingest(wd[0], wl.x_ccs)
        for j, g in enumerate(gold["steps"], start=1):
            assert sha(ws[j - 1]) == g["w_ccs"]
            if check:
                assert pr.check_fresh(FRESH_BOUND(wl)) == set() and pr.last_first_bad == wl.m
            cccs, lc, proof = pr.prove(tr(wl))
            if j < len(ws):
                pr.ingest(wd[j], wl.x_ccs)          # the next instance is on its way before this step's results are examined
            assert sha(cccs[:wl.kappa]) == g["cm"], (j, "cm")
            assert (cccs[wl.kappa:] == wl.x_ccs).all()
            assert sha(proof) == g["proof"], (j, "proof")
            assert sha(lc) == g["lcccs"], (j, "lcccs")
            lc2, f = pr.accumulator()
            assert (lc2 == lc).all() and sha(f) == g["f_ntt"], (j, "f_ntt")
            ok, mx = ctx.linf_check(f, wl.B // 2)
            assert ok and mx == g["norm"], (j, mx, g["norm"])
            ok, lc_v, stage = api.NIFSVerifier.verify(wl, acc, cccs, proof, tr(wl))
            assert ok and (lc_v == lc).all(), (j, stage)
            assert pr.decide(wl.B // 2) == set(), j
            assert pr.steps() == j
            acc = lc
    finally:
        if pr is not None:
            pr.close()
        ctx.close()


# ---- 2, 3: equality with the call-level sequence where no fixture exists ------------------------------------------------------------------------------------
def by_hand(ctx, scheme, wl, ws):
    """the call-level chain with ONE transcript carried across init and the steps -> (acc0, [(cccs, lcccs, proof, f)])"""
    t = tr(wl)
    w_acc = api.Witness.from_w_ccs(ctx, wl.w_ccs)
    acc, _ = api.LFLinearizationProver.prove(ctx, np.concatenate([w_acc.commit(scheme), wl.x_ccs]), w_acc, t)
    acc0, out = acc, []
    for w in ws:
        w_j = api.Witness.from_w_ccs(ctx, w)
        cccs = np.concatenate([w_j.commit(scheme), wl.x_ccs])
        lc, w_next, proof = api.NIFSProver.prove(ctx, acc, w_acc, cccs, w_j, t)
        out.append((cccs, lc, proof, w_next.f))
        w_j.free(); w_acc.free()
        acc, w_acc = lc, w_next
    w_acc.free()
    return acc0, out


SHAPES = {"T8-l2": ("T8", dict(l=2), False), "T8-deg5": ("T8", dict(ccs="deg5"), False), "T8b4": ("T8b4", {}, False), "B6": ("B6", {}, False),
          "T8-extbasis": ("T8", {}, True)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("flags", [0, INLINE])
def test_chain_equals_the_call_level_sequence(shape, flags):
    name, kw, ext = SHAPES[shape]
    wl = make_workload(name, **kw)
    ctx, scheme = setup(wl, random_T(wl.ring, 4242) if ext else None)
    pr = None
    try:
        ws = [np.ascontiguousarray(chain_w_ccs(wl, j)) for j in (1, 2, 3)]
        acc0, want = by_hand(ctx, scheme, wl, ws)
        pr = api.NIFSChainProver(ctx, flags)
        t = tr(wl)
        acc, _ = pr.init(t, wl.w_ccs, wl.x_ccs)
        assert (acc == acc0).all()
        pr.ingest(ws[0], wl.x_ccs)
        for j, (cccs_w, lc_w, proof_w, f_w) in enumerate(want):
            before = t.clone()
            cccs, lc, proof = pr.prove(t)
            if j + 1 < len(ws):
                pr.ingest(ws[j + 1], wl.x_ccs)
            assert (cccs == cccs_w).all() and (lc == lc_w).all() and (proof == proof_w).all(), j
            assert (pr.accumulator()[1] == f_w).all(), j
            if not ext:
                ok, lc_v, stage = api.NIFSVerifier.verify(wl, acc, cccs, proof, before)
                assert ok and (lc_v == lc).all(), (j, stage)
            assert pr.decide(wl.B // 2) == set(), j
            acc = lc
    finally:
        if pr is not None:
            pr.close()
        ctx.close()


# ---- 4: the decider on a tampered accumulator -----------------------------------------------------------------------------------------------------------------
def test_decide_names_the_tampered_component():
    wl = make_workload("T8")
    ctx, _ = setup(wl)
    try:
        pr = api.NIFSChainProver(ctx)
        pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
        pr.ingest(chain_w_ccs(wl, 1), wl.x_ccs)
        pr.prove(tr(wl))
        lc, f = pr.accumulator()
        pr.close()
        u0 = wl.s + wl.tau + wl.kappa                     # lcccs = r[s] v[tau] cm[kappa] u[t] x_w[l] h
        bad = lc.copy()
        bad[u0, 1] = (int(bad[u0, 1]) + 1) % wl.P
        pr = api.NIFSChainProver(ctx)
        pr.resume(bad, f)
        assert pr.decide(wl.B // 2) == {"u"}
        assert "R_LCCCS" in pr.last_error()
        pr.close()
        fc = ctx.icrt(f)                                  # one coefficient word of f moved by one, inside the norm bound
        fc[5, 7] = (int(fc[5, 7]) + 1) % wl.P if int(fc[5, 7]) != wl.B // 2 - 1 else int(fc[5, 7]) - 1
        pr = api.NIFSChainProver(ctx)
        pr.resume(lc, ctx.crt(fc))
        assert pr.decide(wl.B // 2) >= {"cm", "v"}
        pr.close()
    finally:
        ctx.close()


# ---- 5: check_fresh ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, INLINE])
def test_check_fresh(flags):
    wl = make_workload("T8")
    ctx, _ = setup(wl)
    try:
        good = np.ascontiguousarray(chain_w_ccs(wl, 1))
        words = []
        for with_check in (False, True):
            pr = api.NIFSChainProver(ctx, flags)
            pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
            pr.ingest(good, wl.x_ccs)
            if with_check:
                assert pr.check_fresh(FRESH_BOUND(wl)) == set() and pr.last_first_bad == wl.m
                assert pr.check_fresh() == set()          # read-only: the instance stays pending
            words.append(pr.prove(tr(wl)))
            pr.close()
        assert all((a == b).all() for a, b in zip(*words))      # the prove after check_fresh uses the commitment it kept: the same words
        bad = good.copy()
        bad[3, 4] = (int(bad[3, 4]) + 1) % wl.P
        z = np.concatenate([wl.x_ccs, diag(1, wl.ring)[None, :], bad])
        rows = bad_rows(residual_host(wl, z))
        assert len(rows)
        pr = api.NIFSChainProver(ctx, flags)
        pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
        pr.ingest(bad, wl.x_ccs)
        # the commitment is the prover's own (of the tampered witness): lf_cccs_check cannot raise LF_REL_CM, the CCS fails at the host's first bad row
        assert pr.check_fresh(FRESH_BOUND(wl)) == {"ccs"} and pr.last_first_bad == int(rows[0])
        assert "R_CCCS" in pr.last_error()
        pr.close()                                        # (destroyed with the rejected instance still pending)
    finally:
        ctx.close()


# ---- 6: resume ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_form", [False, True])
def test_resume_continues_the_chain_word_for_word(device_form):
    wl = make_workload("T14")
    gold = GOLD["T14"]["steps"]
    ctx, _ = setup(wl)
    try:
        ws = [np.ascontiguousarray(chain_w_ccs(wl, j)) for j in (1, 2, 3)]
        pr = api.NIFSChainProver(ctx)
        pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
        for w in ws:
            pr.ingest(w, wl.x_ccs)
            whole = pr.prove(tr(wl))
        whole_f = pr.accumulator()[1]
        pr.close()
        pr = api.NIFSChainProver(ctx)
        pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
        for w in ws[:2]:
            pr.ingest(w, wl.x_ccs)
            pr.prove(tr(wl))
        if device_form:
            lc, fd = pr.accumulator(out=torch.empty((wl.N, 24), dtype=torch.int64, device="cuda"))
            assert sha(host(fd)) == gold[1]["f_ntt"]
        else:
            lc, fd = pr.accumulator()
        pr.close()
        pr = api.NIFSChainProver(ctx)
        pr.resume(lc, fd)
        assert pr.steps() == 0
        pr.ingest(ws[2], wl.x_ccs)
        again = pr.prove(tr(wl))
        assert all((a == b).all() for a, b in zip(whole, again)) and sha(again[2]) == gold[2]["proof"]
        assert (pr.accumulator()[1] == whole_f).all() and pr.steps() == 1
        pr.close()
    finally:
        ctx.close()


# ---- 7: the state machine and the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_create_refusals():
    wl = make_workload("T8")
    ctx = api.Context(0)
    try:
        assert code_of(lambda: api.NIFSChainProver(ctx)) == E_STATE               # no constraint system
        ctx.load_ccs(wl)
        assert code_of(lambda: api.NIFSChainProver(ctx)) == E_STATE               # no matrix
        api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        assert code_of(lambda: api.NIFSChainProver(ctx, 2)) == E_INVALID          # an unknown flag
        h = C.c_void_p()
        assert api._lib().lf_prover_create(ctx.h, 0, None) == E_INVALID
        api.NIFSChainProver(ctx).close()
    finally:
        ctx.close()
    ctx = api.Context(0)
    try:
        ctx.set_sharding_model(0, 2)                                              # a sharded context (the timing model: no peers needed)
        ctx.load_ccs(wl)
        api.AjtaiCommitmentScheme(ctx, kappa=wl.kappa, n=wl.N, seed=wl.ajtai_seed())
        assert code_of(lambda: api.NIFSChainProver(ctx)) == E_UNSUPPORTED
    finally:
        ctx.close()


def test_state_machine_and_refusals():
    wl = make_workload("T8")
    ctx, scheme = setup(wl)
    L = api._lib()
    try:
        ws = [np.ascontiguousarray(chain_w_ccs(wl, j)) for j in (1, 2)]
        _acc0, want = by_hand(ctx, scheme, wl, ws)
        lc_buf = np.zeros((ctx.lcccs_len, 24), dtype=np.uint64)
        p64 = lambda a: a.ctypes.data_as(api.u64p)
        pr = api.NIFSChainProver(ctx)
        # EMPTY
        for call in (lambda: pr.prove(tr(wl)), lambda: pr.decide(), lambda: pr.accumulator(), lambda: pr.ingest(ws[0], wl.x_ccs), lambda: pr.check_fresh()):
            assert code_of(call) == E_STATE
        assert "lf_prover_" in pr.last_error()
        # NULL arguments
        t = tr(wl)
        assert L.lf_prover_init(pr.h, None, p64(wl.w_ccs), p64(wl.x_ccs), p64(lc_buf), p64(lc_buf)) == E_INVALID
        assert L.lf_prover_init(pr.h, t.h, None, p64(wl.x_ccs), p64(lc_buf), p64(lc_buf)) == E_INVALID
        assert L.lf_prover_resume(pr.h, None, None) == E_INVALID and L.lf_prover_resume_dev(pr.h, p64(lc_buf), None) == E_INVALID
        assert L.lf_prover_ingest(pr.h, None, None) == E_INVALID and L.lf_prover_ingest_dev(pr.h, None, p64(wl.x_ccs)) == E_INVALID
        assert L.lf_prover_check_fresh(pr.h, 0, None, None) == E_INVALID and L.lf_prover_decide(pr.h, 0, None) == E_INVALID
        assert L.lf_prover_prove(pr.h, None, None, None, None) == E_INVALID
        assert L.lf_prover_prove(None, t.h, None, p64(lc_buf), p64(lc_buf)) == E_INVALID and L.lf_prover_decide(None, 0, None) == E_INVALID
        assert code_of(lambda: pr.init(api.PoseidonTranscript(ring="babybear"), wl.w_ccs, wl.x_ccs)) == E_INVALID     # a transcript of the other ring
        # READY
        chain_t = tr(wl)
        pr.init(chain_t, wl.w_ccs, wl.x_ccs)
        assert code_of(lambda: pr.init(tr(wl), wl.w_ccs, wl.x_ccs)) == E_STATE
        lc0, f0 = pr.accumulator()
        assert code_of(lambda: pr.resume(lc0, f0)) == E_STATE and code_of(lambda: pr.resume(lc0, dev(f0))) == E_STATE
        assert code_of(lambda: pr.prove(tr(wl))) == E_STATE and code_of(lambda: pr.check_fresh()) == E_STATE      # nothing pending
        # READY + PENDING: a second ingest is refused; a refusal of ingest / check_fresh / prove drops the pending instance and keeps the accumulator
        pr.ingest(ws[0], wl.x_ccs)
        assert code_of(lambda: pr.ingest(ws[1], wl.x_ccs)) == E_STATE
        assert code_of(lambda: pr.prove(tr(wl))) == E_STATE
        pr.ingest(ws[0], wl.x_ccs)
        assert code_of(lambda: pr.prove(api.PoseidonTranscript(ring="babybear"))) == E_INVALID
        assert pr.decide() == set() and pr.steps() == 0
        # ... and the next good calls give the words of the undisturbed chain
        for w, (cccs_w, lc_w, proof_w, f_w) in zip(ws, want):
            pr.ingest(w, wl.x_ccs)
            cccs, lc, proof = pr.prove(chain_t)
            assert (cccs == cccs_w).all() and (lc == lc_w).all() and (proof == proof_w).all() and (pr.accumulator()[1] == f_w).all()
        assert pr.last_error() == "" and pr.steps() == 2
        # a constraint system loaded again under a live prover (the same one: nothing about its shape changes): every call is refused, nothing is touched
        pr.ingest(ws[0], wl.x_ccs)
        assert pr.check_fresh() == set()            # (joins the ingest job: the constraint system may not be loaded under a running job)
        pr_idle = api.NIFSChainProver(ctx)
        ctx.load_ccs(wl)
        for call in (lambda: pr.prove(tr(wl)), lambda: pr.decide(), lambda: pr.accumulator(), lambda: pr.check_fresh(), lambda: pr_idle.init(tr(wl), wl.w_ccs, wl.x_ccs)):
            assert code_of(call) == E_STATE
        assert "replaced" in pr.last_error() and pr.steps() == 2
        pr.close()                                                                  # destroyed with its instance still pending
        pr_idle.close()
    finally:
        ctx.close()


def test_destroy_with_a_pending_job_leaves_the_context_usable():
    """the job is abandoned by destroy; the context then runs a T8 fold step equal to the CPU oracle"""
    import lfo
    wl = make_workload("T8")
    ctx, scheme = setup(wl)
    try:
        for flags in (0, INLINE):
            pr = api.NIFSChainProver(ctx, flags)
            pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
            pr.ingest(np.ascontiguousarray(chain_w_ccs(wl, 1)), wl.x_ccs)
            pr.close()
        wit = api.Witness.from_w_ccs(ctx, wl.w_ccs)
        cccs = np.concatenate([wit.commit(scheme), wl.x_ccs])
        acc, _ = api.LFLinearizationProver.prove(ctx, cccs, wit, tr(wl))
        lc, w0, proof = api.NIFSProver.prove(ctx, acc, wit, cccs, wit, tr(wl))
        inst = lfo.Instance(wl)
        f_coeff = inst.witness_from_w_ccs(wl.w_ccs)
        acc_o, _ = inst.linearize(lfo.Transcript(), cccs, f_coeff)
        lc_o, f0_o, proof_o = inst.fold_step(lfo.Transcript(), wl.ajtai_matrix(), acc_o, f_coeff, cccs, f_coeff)
        assert (acc == acc_o).all() and (proof == proof_o).all() and (lc == lc_o).all() and (w0.f == f0_o).all()
    finally:
        ctx.close()


# ---- 8: footprint ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, INLINE])
def test_footprint_of_a_chain_in_steady_state(flags):
    """lf_mem_info after step 3 equals that after step 8 (no growth per step); after destroy it equals the value before create.  Freed witness buffers go to the
    library's process-wide recycle pool and the context keeps its scratch buffers, so the measured chain runs after one short chain of the same shape has put the
    pool and the scratch into their steady state: what create .. destroy takes from the device it gives back."""
    wl = make_workload("T14")
    ctx, _ = setup(wl)
    try:
        ws = [np.ascontiguousarray(chain_w_ccs(wl, j)) for j in range(1, 9)]

        def chain(nsteps, marks):
            pr = api.NIFSChainProver(ctx, flags)
            pr.init(tr(wl), wl.w_ccs, wl.x_ccs)
            free = {}
            for j in range(1, nsteps + 1):
                pr.ingest(ws[j - 1], wl.x_ccs)
                pr.prove(tr(wl))
                if j in marks:
                    free[j] = ctx.mem_info()[0]
            pr.close()
            return free

        chain(3, ())
        before = ctx.mem_info()[0]
        free = chain(8, (3, 8))
        assert free[3] == free[8], (free[3] - free[8], "bytes taken between step 3 and step 8")
        assert ctx.mem_info()[0] == before, (before - ctx.mem_info()[0], "bytes not given back")
    finally:
        ctx.close()
