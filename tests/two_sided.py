"""Fold steps whose two sides hold DIFFERENT witnesses: the cases and their oracle references, for tests/test_two_sided_cpu.py (the conditions on the inputs,
on the CPU oracle alone) and tests/test_gpu_two_sided*.py (the device against those references).

A shape is (ring, name, ccs, K, mode): a workload of latticefold_amd.workload.CONFIGS or of SHAPES below, its constraint system, an override of the number of
base-b digits and the digit rule.  A pair names the witness of the left side (the accumulator's) and of the right side (the incoming instance's):

  base    the workload's w_ccs                      chain1 / chain2   chain_w_ccs(wl, 1 / 2): about half of its slots kept, the rest zero
  zero    the all-zero witness                      folded            the folded witness of the oracle's step (base, chain1): dense digits, norm near the bound
  max / min   b = 2: every coefficient of f_coeff +(B/2 - 1) / -(B/2 - 1) (the magnitude planes of the two are equal, the sign planes differ);
              b > 2: w_ccs whose every coefficient is +-sum_i (B/2 - 1) B^i, which witness_from_w_ccs turns into f_coeff = +-(B/2 - 1) everywhere -- the
              largest magnitude it yields in every position at once (it gives +-B/2 only at isolated ties); asserted where the witness is made

Every witness folds under the workload's own constraint system.  base, chain*, zero satisfy it; folded, max and min need not, and neither prover looks: a fold
step never tests satisfaction.  The oracle's side data (f_coeff, commitment, LCCCS) and steps are computed once per key and kept for the process.

Where the kernels choose a side, and the case and switch set (tests/fold_paths.py) that reaches the choice with different data on the two sides:

  lf_rounds.hip   k_fold_round1 (planes, mu_pow)                 every Goldilocks case, "default" and every set without GEMM round 1 / TAB_R1
                  k_fold_round_tab (planes, polynomial tables)   T10, G5, E22, R61, SV10W under "lut + tab" (rounds 1 and 2 as table look-ups)
                  k_fold_round2 (planes, mu_pow)                 every case under "default", "gemm 1", "sv 1"
                  k_fold_materialize2                            every case under "default", "fused fix", "gemm off", the tail sets without look-up tables
                  k_fold_round mode 4 (planes behind a pair)     "lut + tab + FOLD_NO_R4TAB=1"
                  mode 3 and the <NU = false> instantiations     T8 under another non-residue (test_gpu_two_sided.py), "default", "fused fix", "lut + tab ..";
                                                                 on BabyBear only test_gpu_bb.py::test_fold_step_with_another_nonresidue runs them, with one witness
                  mode 5 (round 3 with the mu tables)            every "lut ..", "a3p ..", "gemm .. FOLD_LUT_MIN=1" set
                  mode 6 (round 4, product-free)                 the same sets; split and plain under "a3p .. split / plain"
                  mode 7 (round 5 from the planes)               "a3p m6+m7+m1 ..", "lut + tab + FOLD_R5_MIN=1 ..", "gemm 3 .. FOLD_R5_MIN=1", "tail 64 lut", "tail 16 lut"
                  modes 0 / 1 and k_fold_tail (tables [side K + k])  every case: the tables they read were filled per side by the kernels above
                  k_fold_materialize                             no driver launches it: unreachable, by any test
  lf_sv_rounds.hip  k_sv_gemm (bits[side]), k_sv_finish1 (mu_pow)   T10, G5, E22, R61, SV10W under "gemm ..", "sv ..", "a3p ..": rounds 1, 2 and 3
  lf_fold_i8.hip  k_fold_witness_i8 (planes, rho)                T10, G5, R61, SV10W, T8 under every set but "fold witness valu"
  lf_kernels.hip  k_fold_witness (fw_groups)                     "fold witness valu" on every shape, E22 (K = 22 > 16: the int8 form declines)
                  k_fold_round_g, fold prepare (eqL / eqR, G1 / G2)  every case; theta from coef_eval_dev per side under "theta eval unfused"
  lf_sb.hip       k_sb_round round 1, k_sb_materialize, k_sb_fold_witness   every small-base case; the odd-N edge of the first two on O255b8
  bb_rounds.hip   k_fold_round1 / 2, k_fold_materialize2         BDP, B8 under "default", "fused fix", "gemm 1 / 2"
                  k_fold_round modes 3 .. 7, k_fold_round5_2l    "lut ..", "split ..", "gemm .. FOLD_LUT_MIN=1"
                  k_fold_round_g (eqL / eqR, G1 / G2)            every case
  bb_sv_rounds.hip  the shared k_sv_gemm, k_bbsv_finish (mu_c)    BDP (round 1: 64 pairs), B8 (rounds 1 and 2) under "gemm .."
  bb_kernels.hip  k_fold_witness                                 every BabyBear case

With a side selection made to read the left operand for both sides (one site each in lf_rounds.hip mode 5, lf_sb.hip round 1, bb_rounds.hip modes 3 .. 7), the
one-witness tests of those paths still pass; the cases T10 / T8b4 / B8 (base, chain1) here fail in every section behind the round messages."""
import contextlib
from types import SimpleNamespace

import numpy as np

from latticefold_amd.workload import CONFIGS, chain_w_ccs, make_workload

# (s, wit_len, L, B, b, K, kappa): shapes that other test modules register for themselves under the same names, and the odd-N shape of this one
SHAPES = {
    "R61": (8, 61, 4, 1 << 16, 2, 16, 4),          # tests/test_gpu_q_pack.py: ragged N = 244, n = 63: the int8 dot declines
    "SV10W": (10, 200, 4, 1 << 16, 2, 16, 4),      # tests/test_gpu_sv_gemm_shapes.py: N = 800 of 1024 rows
    "O255b8": (8, 51, 5, 1 << 15, 8, 5, 4),        # N = 255 of m = 256, b = 8: the last pair of round 1 and of k_sb_materialize has one plane entry
}


SWAP = [("base", "chain1"), ("chain1", "base")]
ALL_PAIRS = SWAP + [("base", "zero"), ("zero", "base"), ("folded", "chain2"), ("max", "min"), ("min", "max")]
G, BB = "goldilocks", "babybear"
# (ring, name, ccs, K, mode, pair) of every case of the GPU tests; tests/test_two_sided_cpu.py checks the conditions on each
GOLD_CASES = [(G, "T10", "r1cs", None, 0, p) for p in ALL_PAIRS] + [(G, n, "r1cs", None, 0, p) for n in ("G5", "E22", "R61", "SV10W") for p in SWAP]
BB_CASES = [(BB, n, "r1cs", None, 0, p) for n in ("BDP", "B8") for p in SWAP + [("max", "min")]]
SB_CASES = ([(G, n, "r1cs", None, 0, p) for n in ("T8b4", "T8b16") for p in ALL_PAIRS]
            + [(G, n, "r1cs", None, 0, p) for n in ("T8b8", "R61b4", "R61b16", "O255b8") for p in SWAP]
            + [(G, n, "r1cs", K, 1, p) for n, K in (("T8b4", 9), ("T8b16", 5)) for p in SWAP])
WIDE_CASES = [(G, n, ccs, None, 0, p) for n, ccs in (("T8", "deg7"), ("T10", "mix8")) for p in SWAP]
T8_CASES = [(G, "T8", "r1cs", None, 0, p) for p in SWAP]       # the sub-provers under one transcript, the generic non-residue kernels


def case_id(c):
    ring, name, ccs, K, mode, pair = c
    return f"{name}{'' if ccs == 'r1cs' else '-' + ccs}{'' if K is None else f'-K{K}-rule{mode}'}-{pair[0]}+{pair[1]}"


def oracle_for(ring):
    if ring == "babybear":
        import lfo_bb
        return lfo_bb
    import lfo
    return lfo


def shape_key(ring, name, ccs="r1cs", K=None, mode=0):
    return (ring, name, ccs, K, mode)


def workload(key):
    ring, name, ccs, K, mode = key
    if name in SHAPES:
        with _registered(name):
            wl = make_workload(name, 0, ccs=ccs)
    else:
        wl = make_workload(name, 0, ccs=ccs)
    assert wl.ring == ring
    if K is not None:
        wl.K = K
    return wl


@contextlib.contextmanager
def _registered(name):
    had = CONFIGS.get(name)
    CONFIGS[name] = SHAPES[name]
    try:
        yield
    finally:
        if had is None:
            CONFIGS.pop(name, None)
        else:
            CONFIGS[name] = had


@contextlib.contextmanager
def _rule(O, mode):
    if mode:
        O.set_digit_mode(mode)
    try:
        yield
    finally:
        if mode:
            O.set_digit_mode(0)


def sections(wl, proof):
    """the proof of a fold step cut into its parts (rows of ring elements)"""
    tau = wl.tau
    lin = wl.s * (wl.d + 2) + tau + wl.t
    dec = wl.K * (wl.t + tau + wl.l + 1 + wl.kappa)
    fm = wl.s * (2 * wl.b + 1)
    p = np.asarray(proof).reshape(-1, wl.RE)
    o = lin + 2 * dec
    return {"proof_lin": p[:lin], "proof_dec_left": p[lin:lin + dec], "proof_dec_right": p[lin + dec:o], "proof_fold_msgs": p[o:o + fm],
            "proof_theta": p[o + fm:o + fm + 2 * wl.K * tau], "proof_eta": p[o + fm + 2 * wl.K * tau:], "proof": p}


def section_rows(wl):
    """rows the layout of sections() accounts for: it must be the proof's length"""
    tau = wl.tau
    return (wl.s * (wl.d + 2) + tau + wl.t) + 2 * wl.K * (wl.t + tau + wl.l + 1 + wl.kappa) + wl.s * (2 * wl.b + 1) + 2 * wl.K * tau + 2 * wl.K * wl.t


# ---- the oracle's side of a shape ------------------------------------------------------------------------------------------------------------------------
class OracleShape:
    def __init__(self, key):
        self.key = key
        self.ring, self.name, self.ccs, self.K, self.mode = key
        self.wl = workload(key)
        self.O = oracle_for(self.ring)
        self.inst = self.O.Instance(self.wl)
        self.A = self.wl.ajtai_matrix()
        self._sides, self._steps = {}, {}

    def _commit(self, f):
        O, wl = self.O, self.wl
        return np.concatenate([O.ajtai_commit(self.A, wl.kappa, wl.N, O.crt(f)), wl.x_ccs])

    def w_ccs(self, kind):
        """the w_ccs a kind is ingested from, None where the kind is given as f_coeff"""
        wl, O, P = self.wl, self.O, self.wl.P
        if kind == "base":
            return wl.w_ccs
        if kind in ("chain1", "chain2"):
            return chain_w_ccs(wl, int(kind[-1]))
        if kind == "zero":
            return np.zeros_like(wl.w_ccs)
        if kind in ("max", "min") and wl.b != 2:
            value = sum((wl.B // 2 - 1) * wl.B ** i for i in range(wl.L))
            assert value < P
            return O.crt(np.full((wl.wit_len, wl.RE), value if kind == "max" else P - value, dtype=np.uint64))
        return None

    def side(self, kind):
        """f_coeff, CCCS and LCCCS of a witness kind: SimpleNamespace(f, w_ccs, cccs, acc)"""
        if kind not in self._sides:
            wl, O = self.wl, self.O
            h = wl.B // 2 - 1
            with _rule(O, self.mode):
                w = self.w_ccs(kind)
                if w is not None:
                    f = self.inst.witness_from_w_ccs(w)
                    if kind in ("max", "min"):
                        assert (f == np.uint64(h if kind == "max" else wl.P - h)).all(), (self.key, kind, np.unique(f)[:8])
                elif kind in ("max", "min"):
                    f = np.full((wl.N, wl.RE), h if kind == "max" else wl.P - h, dtype=np.uint64)
                elif kind == "folded":
                    lc, f0, _ = self.step("base", "chain1")
                    f = O.icrt(f0)
                else:
                    raise KeyError(kind)
                cccs = self._commit(f)
                if kind == "folded":
                    acc = lc
                    assert (acc[wl.s + wl.tau:wl.s + wl.tau + wl.kappa] == cccs[:wl.kappa]).all()   # the folded witness opens the folded commitment
                else:
                    acc, _ = self.inst.linearize(O.Transcript(), cccs, f)
            self._sides[kind] = SimpleNamespace(f=f, w_ccs=w, cccs=cccs, acc=acc)
        return self._sides[kind]

    def step(self, left, right):
        """the oracle's (lcccs_out, f0, proof) of the fold step with `left` as the accumulator's witness and `right` as the incoming one"""
        if (left, right) not in self._steps:
            L, R = self.side(left), self.side(right)
            with _rule(self.O, self.mode):
                self._steps[(left, right)] = self.inst.fold_step(self.O.Transcript(), self.A, L.acc, L.f, R.cccs, R.f)
        return self._steps[(left, right)]


_oracle_shapes = {}


def oracle_shape(key):
    if key not in _oracle_shapes:
        _oracle_shapes[key] = OracleShape(key)
    return _oracle_shapes[key]


def reference(ring, name, pair, ccs="r1cs", K=None, mode=0):
    """the oracle alone: SimpleNamespace(wl, shape, L, R, lc, f0, proof) of the step `pair`"""
    sh = oracle_shape(shape_key(ring, name, ccs, K, mode))
    lc, f0, proof = sh.step(*pair)
    return SimpleNamespace(wl=sh.wl, shape=sh, L=sh.side(pair[0]), R=sh.side(pair[1]), lc=lc, f0=f0, proof=proof)


# ---- the device's side -----------------------------------------------------------------------------------------------------------------------------------
class DeviceShape:
    """one context per shape with its constraint system and commitment matrix; the witnesses of the kinds on it, made once"""

    def __init__(self, key, sh=None, ring_tables=None):
        from latticefold_amd import api
        self.api = api
        self.sh = sh or oracle_shape(key)
        self.wl = self.sh.wl
        self.ctx = api.Context(0, ring=self.sh.ring)
        if ring_tables:     # (another non-residue; the caller has given the oracle the same tables and made `sh` under them)
            self.ctx.set_ring_tables(*ring_tables)
        if self.sh.mode:
            self.ctx.set_digit_mode(self.sh.mode)
        self.ctx.load_ccs(self.wl)
        self.scheme = api.AjtaiCommitmentScheme(self.ctx, matrix=self.sh.A)
        self._wits = {}

    def tr(self):
        return self.api.PoseidonTranscript(ring=self.sh.ring)

    def witness(self, kind):
        """the device witness of a kind and its LCCCS, both asserted equal to the oracle's"""
        if kind not in self._wits:
            api, wl, side = self.api, self.wl, self.sh.side(kind)
            if kind == "folded":
                a, b = self.witness("base"), self.witness("chain1")
                lc_o, f0_o, proof_o = self.sh.step("base", "chain1")
                acc, wit, proof = api.NIFSProver.prove(self.ctx, a.acc, a.wit, self.sh.side("chain1").cccs, b.wit, self.tr())
                assert (proof == proof_o).all() and (acc == lc_o).all() and (wit.f == f0_o).all(), (self.sh.key, "the step that makes the folded side")
            else:
                wit = api.Witness.from_w_ccs(self.ctx, side.w_ccs) if side.w_ccs is not None else api.Witness.from_f_coeff(self.ctx, side.f)
                cccs = np.concatenate([wit.commit(self.scheme), wl.x_ccs])
                assert (cccs == side.cccs).all(), (self.sh.key, kind, "commitment")
                acc, _ = api.LFLinearizationProver.prove(self.ctx, cccs, wit, self.tr())
            assert (wit.f_coeff == side.f).all(), (self.sh.key, kind, "f_coeff")
            assert (acc == side.acc).all(), (self.sh.key, kind, "LCCCS")
            self._wits[kind] = SimpleNamespace(wit=wit, acc=acc)
        return self._wits[kind]

    def close(self):
        self._wits.clear()
        self.ctx.close()


_device_shapes = {}


def case(ring, name, pair, ccs="r1cs", K=None, mode=0):
    """SimpleNamespace(wl, ctx, dev, wL, wR, acc, cccs, lc, f0, proof): the workload; the context; the two device witnesses; the linearized accumulator of the
    left one (equal to the oracle's); the CCCS of the right one; the oracle's folded LCCCS, f0 and proof for exactly that pair"""
    key = shape_key(ring, name, ccs, K, mode)
    if key not in _device_shapes:
        _device_shapes[key] = DeviceShape(key)
    dev = _device_shapes[key]
    ref = reference(ring, name, pair, ccs, K, mode)
    L, R = dev.witness(pair[0]), dev.witness(pair[1])
    return SimpleNamespace(wl=dev.wl, ctx=dev.ctx, dev=dev, wL=L.wit, wR=R.wit, acc=L.acc, cccs=ref.R.cccs, lc=ref.lc, f0=ref.f0, proof=ref.proof,
                           O=dev.sh.O, ref=ref)


def case_of(dev, pair):
    """case() on a DeviceShape of the caller's own (not kept here): its oracle shape gives the reference"""
    lc, f0, proof = dev.sh.step(*pair)
    ref = SimpleNamespace(wl=dev.wl, shape=dev.sh, L=dev.sh.side(pair[0]), R=dev.sh.side(pair[1]), lc=lc, f0=f0, proof=proof)
    L, R = dev.witness(pair[0]), dev.witness(pair[1])
    return SimpleNamespace(wl=dev.wl, ctx=dev.ctx, dev=dev, wL=L.wit, wR=R.wit, acc=L.acc, cccs=ref.R.cccs, lc=ref.lc, f0=ref.f0, proof=ref.proof,
                           O=dev.sh.O, ref=ref)


def close_devices():
    for dev in _device_shapes.values():
        dev.close()
    _device_shapes.clear()


def differing(wl, ref, got, what):
    """names of the parts of a step's output (lc, w0, proof) that differ from the reference, word for word: proof per section, folded LCCCS, and f, f_coeff,
    w_ccs of the folded witness as canonical residues"""
    lc, w0, proof = got
    O = oracle_for(wl.ring)
    p = np.uint64(wl.P)
    bad = []
    so, sg = sections(wl, ref.proof), sections(wl, proof)
    bad += [k for k in so if so[k].shape != sg[k].shape or not (so[k] == sg[k]).all()]
    if np.asarray(lc).shape != ref.lc.shape or not (lc == ref.lc).all():
        bad.append("lcccs_out")
    if not hasattr(ref, "w0"):
        f0c = O.icrt(ref.f0)
        ref.w0 = {"f": ref.f0, "f_coeff": f0c, "w_ccs": O.crt(O.recompose(f0c, wl.B, wl.L))}
    want = ref.w0
    have = {"f": np.array(w0.f) % p, "f_coeff": np.array(w0.f_coeff), "w_ccs": np.array(w0.w_ccs) % p}
    bad += ["w0." + k for k in want if have[k].reshape(-1).shape != want[k].reshape(-1).shape or not (have[k].reshape(-1) == want[k].reshape(-1)).all()]
    return [f"{what}: {k}" for k in bad]


def run_sets(c, sets, monkeypatch, expected, applied):
    """one fold step of the case per switch set the shape takes; every difference from the oracle and every path mask that is not the recorded one, by name"""
    from latticefold_amd import api
    wl, bad, ran = c.wl, [], 0
    for ps in sets:
        if not ps.takes(wl.s, wl.N, wl.m):
            continue
        with applied(monkeypatch, ps.env):
            got = api.NIFSProver.prove(c.ctx, c.acc, c.wL, c.cccs, c.wR, c.dev.tr())
        ran += 1
        bad += differing(wl, c.ref, got, ps.name)
        masks = (c.ctx.fold_paths(), c.ctx.fold_split_rounds())
        if masks != expected(ps, wl):
            bad.append(f"{ps.name}: fold_paths / fold_split_rounds {masks} instead of {expected(ps, wl)}")
        got[1].free()
    assert ran > 0
    assert not bad, f"{len(bad)} differences over {ran} switch sets: {bad[:12]}"
