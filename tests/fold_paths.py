"""The environment-switch sets under which the suite drives a fold step, in one place.

The first half holds the dictionaries of the one-witness tests, under the names those tests import them by (tests/test_gpu_fold_a3p.py, three tests of
tests/test_gpu_parity.py, tests/test_gpu_sv_gemm_shapes.py, tests/test_gpu_live_rows.py, tests/test_gpu_bb.py).  The second half flattens them into named
PathSet entries for the two-witness tests (tests/test_gpu_two_sided*.py): every entry knows the ctx.fold_paths() and ctx.fold_split_rounds() a step under it
must report on a shape (s, N, m), and whether the shape can take the path the entry is about at all.

The expectations mirror the drivers' decisions (csrc/lf_fold.cpp FoldB2::rounds_begin / decide_split / dispatch, csrc/bb_prove.cpp BbFold::rounds_begin /
decide_split) for an unsharded context on the default ring tables; tests/test_two_sided_cpu.py holds them against the formulas the one-witness tests assert.
Nothing here needs a GPU."""
from contextlib import contextmanager

# ---- tests/test_gpu_fold_a3p.py ------------------------------------------------------------------------------------------------------------------------
# rounds 1..3 as GEMMs (the split form of the table rounds hangs on their eq tables), rounds 4.. per launch from the digit look-up tables / with the fused fix
A3P_BASE = {"LF_FOLD_SV_MIN": "64", "LF_DOT_MIN": "64", "LF_FOLD_SV_ROUNDS": "3", "LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_NO_TAIL": "1"}
# name -> (switches, round 5 on the planes?, split form asked for?)
#   round 4 is mode 6 in every case (storing its tables only when round 5 does not run on the planes); round 5 is mode 7 or the fused fix (mode 1); rounds 6.. mode 1,
#   which the driver never runs in the split form
A3P_PATHS = {
    "m6+m7+m1 split": ({"LF_FOLD_R5_MIN": "1", "LF_FOLD_SPLIT_MIN": "1"}, True, True),
    "m6+m7+m1 plain": ({"LF_FOLD_R5_MIN": "1", "LF_FOLD_ROUNDS_NO_SPLIT": "1"}, True, False),
    "m6(stored)+m1 split": ({"LF_FOLD_NO_R5TAB": "1", "LF_FOLD_SPLIT_MIN": "1"}, False, True),
    "m6(stored)+m1 plain": ({"LF_FOLD_NO_R5TAB": "1", "LF_FOLD_ROUNDS_NO_SPLIT": "1"}, False, False),
}

# ---- tests/test_gpu_parity.py::test_fold_step_fused_fix_rounds_match_oracle ------------------------------------------------------------------------------
FUSED_TAIL_OFF = {"LF_NO_TAIL": "1"}                                             # per-round launches for every round, through the whole test
FUSED_FIX = {"LF_FOLD_FUSE_MIN": "4", "LF_FOLD_NO_LUT": "1"}                     # rounds >= 4 with the fix fused in, f-hat materialised after round 2
# rounds 3 and 4 from the 81-entry digit look-up table, rounds 1-2 as gathers from the per-table coefficient tables
FUSED_LUT_TAB = {"LF_FOLD_FUSE_MIN": "4", "LF_FOLD_LUT_MIN": "1", "LF_FOLD_TAB_MIN": "1", "LF_FOLD_TAB_R1": "1"}
# on top of FUSED_LUT_TAB: the product-free forms of rounds 4 and 5 (modes 6 and 7), round 5 on the planes / on the stored round-4 tables / the older modes 4 and 1
FUSED_LUT_EXTRAS = ({"LF_FOLD_R5_MIN": "1"}, {"LF_FOLD_R5_MIN": "1", "LF_FOLD_SPLIT_MIN": "1"}, {"LF_FOLD_NO_R5TAB": "1"},
                    {"LF_FOLD_NO_R5TAB": "1", "LF_FOLD_SPLIT_MIN": "1"}, {"LF_FOLD_NO_R4TAB": "1"})
# the separate k_fix pass, theta from evaluate_mles-style sums, likewise u of the linearization
UNFUSED_EVAL = {"LF_FOLD_UNFUSED": "1", "LF_THETA_EVAL": "1", "LF_LIN_U_EVAL": "1"}

# ---- tests/test_gpu_parity.py::test_fold_step_gemm_rounds_match_oracle -----------------------------------------------------------------------------------
GEMM_BASE = {"LF_FOLD_SV_MIN": "64", "LF_DOT_MIN": "64"}                         # ... and the u_s / eta inner products as int8 GEMMs at this size too
# (LF_FOLD_SV_ROUNDS, further switches)
GEMM_CASES = ((1, {}), (2, {}), (3, {}), (2, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4"}), (3, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4"}),
              (3, {"LF_NO_TAIL": "1", "LF_FOLD_UNFUSED": "1"}), (3, {"LF_FOLD_SV_NO_SPLIT": "1"}),
              (3, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_R5_MIN": "1", "LF_NO_TAIL": "1", "LF_FOLD_SPLIT_MIN": "1"}),
              (3, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_R5_MIN": "1", "LF_NO_TAIL": "1", "LF_FOLD_ROUNDS_NO_SPLIT": "1"}),
              (2, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_NO_R5TAB": "1", "LF_FOLD_ROUNDS_NO_SPLIT": "1"}))
GEMM_OFF = {"LF_FOLD_NO_SV": "1"}

# ---- tests/test_gpu_parity.py::test_fold_step_persistent_tail_matches_oracle -----------------------------------------------------------------------------
# (LF_TAIL_N, look-up-table rounds before the tail?)
TAIL_CASES = (("16384", False), ("16", False), ("4", False), ("64", True), ("16", True), ("0", False))
TAIL_LUT = {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_R5_MIN": "1"}
TAIL_DEVICE_TRANSCRIPT = {"LF_DEVICE_TRANSCRIPT": "1"}
TAIL_DEVICE_TRANSCRIPT_N = ("16384", "16")

# ---- tests/test_gpu_sv_gemm_shapes.py::gemm_rounds -------------------------------------------------------------------------------------------------------
SV_MIN = {"LF_FOLD_SV_MIN": "64"}
SV_DOT_MIN = {"LF_DOT_MIN": "64"}
SV_ROUNDS = (1, 2, 3)
SV_FORMS = ({}, {"LF_FOLD_SV_NO_SPLIT": "1"})

# ---- tests/test_gpu_live_rows.py -------------------------------------------------------------------------------------------------------------------------
LIVE_TAIL_N = 64
LIVE_LOW = {"LF_LIVE_ROWS_LOW": "1", "LF_TAIL_N": str(LIVE_TAIL_N)}
LIVE_SPLIT = dict(LIVE_LOW, LF_LIN_SPLIT_MIN="16")
LIVE_OFF = {"LF_NO_LIVE_ROWS": "1"}

# ---- tests/test_gpu_bb.py --------------------------------------------------------------------------------------------------------------------------------
BB_FUSED_FIX = {"LF_FOLD_FUSE_MIN": "4", "LF_FOLD_NO_LUT": "1"}
BB_FUSED_LUT = {"LF_FOLD_FUSE_MIN": "4", "LF_FOLD_LUT_MIN": "1"}
BB_FUSED_LUT_EXTRAS = ({"LF_FOLD_R5_MIN": "1"}, {"LF_FOLD_NO_R5TAB": "1"}, {"LF_FOLD_NO_R4TAB": "1"})
BB_GEMM_BASE = {"LF_FOLD_SV_MIN": "64"}
BB_GEMM_CASES = ((1, {}), (2, {}), (3, {}), (3, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4"}),
                 (2, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_R5_MIN": "1"}),
                 (3, {"LF_FOLD_UNFUSED": "1"}), (3, {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_NO_R4TAB": "1"}))
BB_SPLIT_BASE = {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4", "LF_FOLD_SPLIT_MIN": "1"}
# (further switches, the split mask where the shape has a round 5)
BB_SPLIT_CASES = (({}, 0b01000), ({"LF_FOLD_R5_MIN": "1"}, 0b01000), ({"LF_FOLD_R5_MIN": "1", "LF_FOLD_SV_MIN": "64"}, 0b01000),
                  ({"LF_FOLD_R5_MIN": "1", "LF_FOLD_ROUNDS_NO_SPLIT": "1"}, 0), ({"LF_FOLD_NO_R4TAB": "1"}, 0))
BB_DOT_I8 = {"LF_DOT_MIN": "64"}
BB_DOT_VALU = {"LF_DOT_MIN": "64", "LF_DOT_VALU": "1"}
BB_NU_LUT = {"LF_FOLD_LUT_MIN": "1", "LF_FOLD_FUSE_MIN": "4"}                     # test_fold_step_with_another_nonresidue
BB_NU_LUT_R5 = dict(BB_NU_LUT, LF_FOLD_R5_MIN="1")


@contextmanager
def applied(monkeypatch, *envs):
    """the switches of `envs` set for the body, the environment as it was afterwards"""
    with monkeypatch.context() as mp:
        for env in envs:
            for k, v in env.items():
                mp.setenv(k, v)
        yield


# ==== what a step under a set of switches must report =====================================================================================================
def _int(env, key, default):
    return int(env[key]) if key in env else default


def decisions(ring, env, s, N, m):
    """the driver's choices for one unsharded b = 2 fold step on a shape: which rounds run as int8 GEMMs (`gemm`, the mask of ctx.fold_paths()), which table
    rounds run in the split eq form (`split`, the mask of ctx.fold_split_rounds()), and the round modes the look-up tables make possible"""
    bb = ring == "babybear"
    on = lambda k: k in env
    sv_min = _int(env, "LF_FOLD_SV_MIN", 65536)
    if bb and sv_min >= 65536:
        sv_min = 16384
    sv_rounds = _int(env, "LF_FOLD_SV_ROUNDS", 3)
    tail_n = _int(env, "LF_TAIL_N", 2048)
    lut_min = _int(env, "LF_FOLD_LUT_MIN", 1 << 14)           # (the rings' defaults differ, both far above the shapes of the suite)
    r5_min = _int(env, "LF_FOLD_R5_MIN", 8192)
    split_min = _int(env, "LF_FOLD_SPLIT_MIN", 8192)
    fused = not on("LF_FOLD_UNFUSED")
    use_lut = fused and s >= 4 and m // 4 >= lut_min and m // 4 >= 4 and not on("LF_FOLD_NO_LUT")
    use_r4tab = use_lut and not on("LF_FOLD_NO_R4TAB")
    use_r5 = use_r4tab and not on("LF_FOLD_NO_R5TAB") and s >= 5 and N % 4 == 0 and m // 32 >= r5_min
    if not bb:
        use_r5 = use_r5 and (on("LF_NO_TAIL") or m // 8 > tail_n)
    use_sv = not on("LF_FOLD_NO_SV") and N <= m and N % 4 == 0
    use_sv = use_sv and (s >= 4 if bb else not on("LF_FOLD_TAB_R1"))
    gemm = 0
    if use_sv:
        for r in range(1, min(sv_rounds, 3) + 1):
            pairs = m >> r
            if pairs >= sv_min and pairs >= 64 and pairs % 16 == 0:
                gemm |= 1 << (r - 1)
    split = 0
    if bb:
        fr_split = not on("LF_FOLD_ROUNDS_NO_SPLIT") and s >= 5
        if fr_split and use_r4tab and (m >> 4) >= split_min:       # (round 5 from the planes runs unsplit on two lanes per pair)
            split |= 0b01000
    else:
        fr_split = not on("LF_FOLD_SV_NO_SPLIT") and s >= 4 and m >= 256 and not on("LF_FOLD_ROUNDS_NO_SPLIT")
        if fr_split and use_r4tab and (m >> 4) >= split_min:
            split |= 0b01000
        if fr_split and use_r5 and (m >> 5) >= split_min:
            split |= 0b10000
    return {"gemm": gemm, "split": split, "lut": use_lut, "r4tab": use_r4tab, "mode7": use_r5, "fused": fused,
            "tail": not bb and not on("LF_NO_TAIL") and s >= 5 and tail_n >= 4, "any": True}


class PathSet:
    """one named set of switches; `wants` names the decision (a key of decisions()) the set exists to reach: a shape that cannot take it skips the set"""

    def __init__(self, name, env, ring="goldilocks", wants="any"):
        self.name, self.env, self.ring, self.wants = name, dict(env), ring, wants

    def paths(self, s, N, m):
        return decisions(self.ring, self.env, s, N, m)["gemm"]

    def split(self, s, N, m):
        return decisions(self.ring, self.env, s, N, m)["split"]

    def takes(self, s, N, m):
        return bool(decisions(self.ring, self.env, s, N, m)[self.wants])

    def __repr__(self):
        return f"PathSet({self.name})"


def _label(env):
    return " ".join(f"{k[3:]}={v}" for k, v in env.items()) or "default"


def _unique(sets):
    seen, out = set(), []
    for ps in sets:
        key = tuple(sorted(ps.env.items()))
        if key not in seen:
            seen.add(key)
            out.append(ps)
    return out


def _gold_sets():
    S = [PathSet("default", {})]
    S += [PathSet(f"a3p {k}", dict(A3P_BASE, **extra), wants="mode7" if r5 else "r4tab") for k, (extra, r5, _) in A3P_PATHS.items()]
    S.append(PathSet("a3p base", A3P_BASE, wants="r4tab"))
    S.append(PathSet("fused fix", dict(FUSED_TAIL_OFF, **FUSED_FIX), wants="fused"))
    S.append(PathSet("lut + tab", dict(FUSED_TAIL_OFF, **FUSED_LUT_TAB), wants="lut"))
    S += [PathSet("lut + tab + " + _label(e), dict(FUSED_TAIL_OFF, **FUSED_LUT_TAB, **e), wants="lut") for e in FUSED_LUT_EXTRAS]
    S.append(PathSet("unfused, theta / u evaluated", dict(FUSED_TAIL_OFF, **UNFUSED_EVAL)))
    S += [PathSet(f"gemm {r} " + _label(e), dict(GEMM_BASE, LF_FOLD_SV_ROUNDS=str(r), **e), wants="gemm") for r, e in GEMM_CASES]
    S.append(PathSet("gemm off", dict(GEMM_BASE, LF_FOLD_SV_ROUNDS="2", **GEMM_OFF)))
    S += [PathSet(f"tail {n}" + (" lut" if lut else ""), dict({"LF_TAIL_N": n}, **(TAIL_LUT if lut else {})), wants="tail" if int(n) >= 4 else "any")
          for n, lut in TAIL_CASES]
    S += [PathSet(f"tail {n} device transcript", dict(TAIL_DEVICE_TRANSCRIPT, LF_TAIL_N=n), wants="tail") for n in TAIL_DEVICE_TRANSCRIPT_N]
    S += [PathSet(f"sv {r} " + _label(f), dict(SV_MIN, **SV_DOT_MIN, LF_FOLD_SV_ROUNDS=str(r), **f), wants="gemm") for r in SV_ROUNDS for f in SV_FORMS]
    S += [PathSet("live low", LIVE_LOW), PathSet("live low, whole tables", dict(LIVE_LOW, **LIVE_OFF)),
          PathSet("live split", LIVE_SPLIT), PathSet("live split, whole tables", dict(LIVE_SPLIT, **LIVE_OFF))]
    # the switches of the two-witness tests' own list
    S += [PathSet("fold witness valu", {"LF_FOLD_WITNESS_VALU": "1"}), PathSet("zk valu", {"LF_ZK_VALU": "1"}), PathSet("dot valu", {"LF_DOT_VALU": "1"}),
          PathSet("dot i8", {"LF_DOT_MIN": "64"}), PathSet("q two pass", {"LF_DOT_MIN": "64", "LF_Q_TWO_PASS": "1"}),
          PathSet("theta eval unfused", {"LF_THETA_EVAL": "1", "LF_FOLD_UNFUSED": "1"}), PathSet("live rows low", {"LF_LIVE_ROWS_LOW": "1"}),
          PathSet("no live rows", LIVE_OFF)]
    return _unique(S)


def _bb_sets():
    R = "babybear"
    S = [PathSet("default", {}, R)]
    S.append(PathSet("fused fix", BB_FUSED_FIX, R, "fused"))
    S.append(PathSet("lut", BB_FUSED_LUT, R, "lut"))
    S += [PathSet("lut + " + _label(e), dict(BB_FUSED_LUT, **e), R, "lut") for e in BB_FUSED_LUT_EXTRAS]
    S.append(PathSet("unfused, theta / u evaluated", UNFUSED_EVAL, R))
    S += [PathSet(f"gemm {r} " + _label(e), dict(BB_GEMM_BASE, LF_FOLD_SV_ROUNDS=str(r), **e), R, "gemm") for r, e in BB_GEMM_CASES]
    S.append(PathSet("gemm off", dict(BB_GEMM_BASE, LF_FOLD_SV_ROUNDS="3", **GEMM_OFF), R))
    S += [PathSet("split " + _label(e), dict(BB_SPLIT_BASE, **e), R, "lut") for e, _ in BB_SPLIT_CASES]
    S += [PathSet("dot i8", BB_DOT_I8, R), PathSet("dot valu", BB_DOT_VALU, R)]
    return _unique(S)


GOLD_SETS = _gold_sets()
BB_SETS = _bb_sets()
# the small-base path (csrc/lf_fold_sb.cpp) reads none of the round switches: one lane, ordinary launches.  What it shares with the b = 2 path and a switch
# reaches: the inner products, M z over the live rows, the z_k build.  It never runs GEMM or split rounds: both masks are 0.
SB_SETS = [PathSet("default", {}), PathSet("dot i8", {"LF_DOT_MIN": "64"}), PathSet("dot valu", {"LF_DOT_VALU": "1"}), PathSet("zk valu", {"LF_ZK_VALU": "1"}),
           PathSet("live rows low", {"LF_LIVE_ROWS_LOW": "1"}), PathSet("no live rows", LIVE_OFF)]


def expected(ps, wl):
    """(fold_paths, fold_split_rounds) of a step under `ps` on the workload; b > 2 and wide constraint systems never take GEMM or split rounds"""
    if wl.b != 2:
        return 0, 0
    return ps.paths(wl.s, wl.N, wl.m), ps.split(wl.s, wl.N, wl.m)
