"""The flat PlusProof and the host-only verifier object of the C ABI (lfplus_proof_len / lfplus_proof_layout / lfplus_verify: csrc/lfp_prover.cpp), without a
GPU: lengths and layout against the field sizes of the oracle's proofs, lfplus_verify on oracle proofs (accept, the closing challenge, tampering per section
with the stages plus.PlusVerifier reports, malformed buffers), and the names of the Rust `plus` module against the reference's."""
import ctypes as C
import json
import os
import re
from math import ceil, log, sqrt

import numpy as np
import pytest

import lfp
from latticefold_amd import plus

D, P = 16, plus.P
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N = 1 << 15
ELL = ceil(log(P) / log(8))


def _bound(L, k):
    a, c = 16 * 128 * L, 8 + 16 * k + 1                  # utils::estimate_bound (utils.rs:102-112)
    return ceil((a + sqrt(a * a + 4 * a * c)) / 2)


_CASES = {}


def _case(kappa, k, rounds):
    """the oracle's PlusProver over `rounds` fresh instances per prove, once per shape: (params, r1cs, [(proof dict, L, nfresh)])"""
    key = (kappa, k, rounds)
    if key not in _CASES:
        B = _bound(3, k) + 1 if k == 2 else _bound(3, k) // 2
        A = lfp.splitmix(22, 0, kappa * N * D).reshape(kappa, N, D)
        r1cs = plus.r1cs_decomposed_square((plus.identity_csr(N // k),) * 3, N, B, k)
        params = plus.PlusParameters(plus.LinParameters(kappa, plus.DecompParameters(8, k, ELL)), B)
        oracle = lfp.PlusOracle(A, list(r1cs), kappa, 8, k, ELL, B, lfp.Transcript())
        rng, runs, nacc = np.random.default_rng(6), [], 0
        for ncomp in rounds:
            zs = []
            for _ in range(ncomp):
                z = np.zeros((N // k, D), dtype=np.uint64)
                z[:, 0] = rng.integers(0, 2, size=N // k)
                zs.append(z)
            proof = oracle.prove([(lfp.gadget_decompose(z, B, k), r1cs) for z in zs])
            runs.append((proof, nacc + ncomp, ncomp))
            nacc = 2
        _CASES[key] = (params, runs)
    return _CASES[key]


def _sizes(proof):
    """the field sizes of a proof dict in the documented order"""
    out = []
    for lp in proof["lproof"]:
        out += [np.asarray(lp[key]).size for key in ("msgs", "r", "evals")]
    out += [np.asarray(proof["cmproof"][key]).size for key in plus.PROOF_CM_KEYS]
    out += [np.asarray(proof["linb2x"][key]).size for key in ("cm_g", "ro", "vo")]
    out += [np.asarray(proof["dproof"][key]).size for key in ("C0", "C1", "v0", "v1")]
    return out


def test_proof_len_and_layout_match_the_oracles_field_sizes():
    """Three parameter sets -- (kappa 1, k 4) first prove (L = nfresh = 2) and accumulating prove (L = 3, nfresh = 1), (kappa 2, k 2) first prove: lfplus_proof_len
    = header + the sum of the oracle proof's field sizes; lfplus_proof_layout is contiguous from the header on, in the documented order, with those sizes"""
    seen = 0
    for kappa, k, rounds in ((1, 4, (2, 1)), (2, 2, (2,))):
        params, runs = _case(kappa, k, rounds)
        for proof, L, nfresh in runs:
            sizes = _sizes(proof)
            assert plus.proof_len(params, N, 3, L, nfresh) == plus.PROOF_HEADER + sum(sizes)
            off, ln = plus.proof_layout(params, N, 3, L, nfresh)
            assert ln == sizes and len(off) == 3 * nfresh + 24 == plus._nlib().lfplus_proof_fields(nfresh)
            assert off[0] == plus.PROOF_HEADER and all(off[i + 1] == off[i] + ln[i] for i in range(len(off) - 1))
            assert [int(np.prod(s)) for _, s in plus.proof_fields(params, N, 3, L, nfresh)] == sizes
            flat = plus.proof_to_flat(proof, params, N, 3)
            assert flat.size == plus.proof_len(params, N, 3, L, nfresh) and (flat < np.uint64(P)).all()
            back = plus.proof_from_flat(flat, params, N, 3, L, nfresh)
            for (path, _), size in zip(plus.proof_fields(params, N, 3, L, nfresh), sizes):
                src = proof["lproof"][path[1]] if path[0] == "lproof" else proof[path[0]]
                dst = back["lproof"][path[1]] if path[0] == "lproof" else back[path[0]]
                assert (np.asarray(src[path[-1]]).reshape(-1) == dst[path[-1]].reshape(-1)).all(), path
            seen += 1
    assert seen == 3
    # outside the envelope: length 0, layout refused
    params = _case(1, 4, (2, 1))[0]
    assert plus.proof_len(params, N + 1, 3, 2, 2) == 0 and plus.proof_len(params, N, 3, 1, 2) == 0 and plus.proof_len(params, N, 65, 2, 2) == 0
    with pytest.raises(plus.LfPlusError) as e:
        plus.proof_layout(params, N, 3, 0, 0)
    assert e.value.code == plus.E_ARG


def test_lfplus_verify_accepts_oracle_proofs_without_a_gpu():
    """two chained oracle proves through NativePlusVerifier (lfplus_verify) on ONE transcript: accepted, and the transcript's next challenge is the oracle
    verifier's"""
    params, runs = _case(1, 4, (2, 1))
    ver, ts_o = plus.NativePlusVerifier.init((1, N, D), [None] * 3, params, plus.PoseidonTranscript()), lfp.Transcript()
    for proof, L, nfresh in runs:
        assert ver.verify(plus.proof_to_flat(proof, params, N, 3), L, nfresh), ver.stage
        assert ver.stage is None and ver.code == 0
        assert lfp.plus_verify(ts_o, proof, params.B) == 0
    assert ver.transcript.get_challenge() == ts_o.challenge()


def test_tampering_is_rejected_per_section_with_the_python_verifiers_stage():
    """one word changed in an lproof message, a cmproof field, dproof.C0 and dproof.v1: LFPLUS_E_REJECT with the (which, stage) plus.PlusVerifier reports for
    the same proof as a dict"""
    params, runs = _case(1, 4, (2, 1))
    proof, L, nfresh = runs[0]
    flat = plus.proof_to_flat(proof, params, N, 3)
    off, _ = plus.proof_layout(params, N, 3, L, nfresh)
    index = {path: o for (path, _), o in zip(plus.proof_fields(params, N, 3, L, nfresh), off)}
    A_shape = np.zeros((1, N, D), dtype=np.uint8)
    for path, word, want_which in ((("lproof", 1, "msgs"), 2 * 4 * D + D, 1), (("cmproof", "pb"), 4 * 3 * D + D + 2, nfresh), (("dproof", "C0"), 5, nfresh + 1),
                                   (("dproof", "v1"), 2 * D + 3, nfresh + 1)):
        bad = flat.copy()
        bad[index[path] + word] = (int(bad[index[path] + word]) + 1) % P
        nv = plus.NativePlusVerifier.init((1, N, D), [None] * 3, params, plus.PoseidonTranscript())
        assert not nv.verify(bad, L, nfresh) and nv.code == plus.E_REJECT and nv.which == want_which, (path, nv.stage)
        pv = plus.PlusVerifier.init(A_shape, [None] * 3, params, plus.PoseidonTranscript())
        assert not pv.verify(plus.proof_from_flat(bad, params, N, 3, L, nfresh))
        assert nv.stage == pv.stage, (path, nv.stage, pv.stage)


def test_malformed_buffers_are_refused_before_a_field_is_read():
    """a buffer one word short / long, a header whose L or kappa disagrees with the arguments, proof == NULL: LFPLUS_E_ARG, and the transcript has not moved
    (no sub-verifier ran).  The short buffer is an exact-size allocation: a verifier that sized anything from the header or read on would run off its end."""
    params, runs = _case(1, 4, (2, 1))
    proof, L, nfresh = runs[0]
    flat = plus.proof_to_flat(proof, params, N, 3)
    fresh = plus.PoseidonTranscript().get_challenge()

    def refused(words, L_=L, nfresh_=nfresh, params_=params):
        tr = plus.PoseidonTranscript()
        nv = plus.NativePlusVerifier.init((params_.lin.kappa, N, D), [None] * 3, params_, tr)
        assert not nv.verify(words, L_, nfresh_)
        assert nv.code == plus.E_ARG and nv.stage[0] == "malformed" and nv.which == -1
        assert tr.get_challenge() == fresh
    refused(flat[:-1].copy())
    refused(np.concatenate([flat, np.zeros(1, dtype=np.uint64)]))
    for pos in (1, 6):                                   # header words: L, kappa
        bad = flat.copy()
        bad[pos] += np.uint64(1)
        refused(bad)
    refused(flat, L_=L + 1)                              # the verifier's statement wins: right buffer, other L -> other length
    p2 = plus.PlusParameters(plus.LinParameters(2, params.lin.decomp), params.B)
    refused(flat, params_=p2)
    refused(None)
    # a buffer of the length the LYING header would imply (kappa 2) under the verifier's kappa 1
    lie = np.zeros(plus.proof_len(p2, N, 3, L, nfresh), dtype=np.uint64)
    lie[:plus.PROOF_HEADER] = plus._proof_header(p2, N, 3, L, nfresh)
    refused(lie)
    # raw call: NULL transcript, NULL params
    lib = plus._nlib()
    w, st = C.c_int(), C.c_int()
    assert lib.lfplus_verify(C.byref(plus._cparams(params)), N, 3, L, nfresh, None, flat.ctypes.data_as(plus.u64p), flat.size, C.byref(w), C.byref(st)) == plus.E_ARG
    assert lib.lfplus_verify(None, N, 3, L, nfresh, plus.PoseidonTranscript().h, flat.ctypes.data_as(plus.u64p), flat.size, None, None) == plus.E_ARG
    # proof_to_flat / proof_from_flat refuse what does not fit, as the dict verifier's _shaped does
    short = dict(proof, dproof=dict(proof["dproof"], v1=np.asarray(proof["dproof"]["v1"])[:-1]))
    with pytest.raises(plus.LfPlusError) as e:
        plus.proof_to_flat(short, params, N, 3)
    assert e.value.code == plus.E_ARG
    with pytest.raises(plus.LfPlusError):
        plus.proof_from_flat(flat[:-1], params, N, 3, L, nfresh)


def test_malformed_buffers_under_the_address_and_undefined_sanitizers():
    """the same cases once more against a host-only build of lfp_prover.cpp with -fsanitize=address,undefined (`make asan-verify`: a stand-alone program,
    csrc/lfp_verify_selftest.cpp, over exact-size heap buffers; the sub-verifiers come from the ordinary library): every case gives its code and neither
    sanitizer reports anything"""
    import subprocess
    csrc = os.path.join(ROOT, "latticefold_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "asan-verify"], check=True, capture_output=True, text=True)
    run = subprocess.run([os.path.join(csrc, "build", "lfp_verify_selftest")], capture_output=True, text=True)
    out = run.stdout + run.stderr
    assert run.returncode == 0 and "selftest ok" in run.stdout, out
    assert "Sanitizer" not in out and "runtime error" not in out and "UNEXPECTED" not in out, out
    for case in ("one word short", "one word long", "header L + 1", "header kappa + 1", "NULL proof"):
        assert re.search(re.escape(case) + r"\s+rc = -1\b", run.stdout), (case, out)


# ---- bindings/latticefold-hip/src/plus.rs (never compiled here: names and arities only, as tests/test_rust_wrapper_cpu.py) ----------------------------------
def _params(sig):
    depth, cur, out = 0, "", []
    for ch in sig:
        if ch in "(<[":
            depth += 1
        elif ch in ")>]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return [p.split(":")[0].strip().lstrip("&").replace("mut ", "").strip() for p in out if ":" in p]


def _fn_sig(text, owner_pat, name):
    m = re.search(owner_pat, text, re.S)
    assert m, owner_pat
    body = text[m.end():]
    f = re.search(r"pub fn\s+" + name + r"\s*(?:<[^>]*>)?\s*\(", body)
    assert f, (owner_pat, name)
    depth, i = 1, f.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(body[i], 0)
        i += 1
    return [p for p in _params(body[f.end():i - 1]) if p != "self"]


def test_rust_plus_module_carries_the_reference_names():
    """HipPlusProver::{init, prove} / HipPlusVerifier::{init, verify} have the parameter names and counts of plus.rs:55-61, 77, 118-123, 133 (recorded in
    tests/golden/lfplus_reference_signatures.json: names only); PlusProof is a newtype over the flat words; the error type carries the LFPLUS_E_* code; every
    sys:: function the module calls is declared by the -sys crate and exported by the library"""
    src = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "plus.rs")).read()
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "lfplus_reference_signatures.json")))
    assert re.search(r"^pub mod plus;", open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read(), re.M)
    for owner, fns in ref["methods"].items():
        for name, want in fns.items():
            got = [p.lstrip("_") for p in _fn_sig(src, r"impl[^{]*\bHip" + owner + r"\b[^{]*\{", name)]
            assert got == want, (owner, name, got, want)
    assert re.search(r"pub struct PlusProof\(\s*pub Vec<u64>\s*\)", src)
    assert re.search(r"pub struct HipPlusError\s*\{[^}]*pub code: i32", src, re.S)
    for code in ("LFPLUS_E_ARG", "LFPLUS_E_REJECT"):
        assert "sys::" + code in src
    sysrs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    declared = set(re.findall(r"pub fn (lfplus_[a-z0-9_]+)\(", sysrs))
    used = set(re.findall(r"sys::(lfplus_[a-z0-9_]+)\(", src))
    assert {"lfplus_prover_create", "lfplus_prover_destroy", "lfplus_prover_set_instances", "lfplus_prover_prove", "lfplus_verify", "lfplus_proof_len"} <= used <= declared
    lib = plus._lib()
    assert all(hasattr(lib, s) for s in used)
