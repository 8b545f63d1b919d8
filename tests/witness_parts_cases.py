"""Shapes and inputs shared by test_witness_parts_cpu.py and test_gpu_witness_parts.py: the decomposed witnesses of lf_witness_decompose / lf_witness_recompose.
Not a test module."""
import numpy as np

from latticefold_amd.workload import make_workload, splitmix_fq

# (workload, K override, digit rule).  T8: N 256; G5: N 320, K 15, L 5; R61b4: ragged N 244; T8b8 / T8b16: small bases; (T8b4, 9) / (T8b16, 5): rule 1 needs one
# digit more at b > 2; E31 / E32: K 31 / 32 (E32 reaches -2^31); B6 / BDP / B333: BabyBear, B333 with N 666 = 2 mod 4.  b = 2 cuts the same under either rule:
# T8 and B6 run under both
CASES = [("T8", None, 0), ("T8", None, 1), ("G5", None, 0), ("R61b4", None, 0), ("T8b8", None, 0), ("T8b16", None, 0), ("T8b4", 9, 1), ("T8b16", 5, 1),
         ("E31", None, 0), ("E32", None, 0), ("B6", None, 0), ("B6", None, 1), ("BDP", None, 0), ("B333", None, 0)]
CASE_IDS = [f"{n}{'' if k is None else '-K%d' % k}-rule{m}" for n, k, m in CASES]


def workload(name, K=None):
    wl = make_workload(name, 0)
    if K is not None:
        wl.K = K
    return wl


def oracle_for(wl):
    """the CPU oracle built for the workload's ring"""
    if wl.ring == "babybear":
        import lfo_bb
        return lfo_bb
    import lfo
    return lfo


def digits_cover(b, K, B, mode):
    """K balanced base-b digits reach every |v| <= B/2 under the rule (include/lfhip.h, lf_params)"""
    geo = (b**K - 1) // (b - 1)
    if b == 2:
        return geo >= B // 2
    return (b // 2 if mode == 0 else b // 2 - 1) * geo >= B // 2


def centred(a, P):
    """canonical residues -> Python integers in (-P/2, P/2]"""
    a = np.asarray(a, dtype=np.uint64).astype(object)
    return np.where(a > (P - 1) // 2, a - P, a)


def residues(v, P):
    """centred int64 values -> canonical residues"""
    v = np.asarray(v, dtype=np.int64)
    return np.where(v < 0, np.uint64(P) - (-v).astype(np.uint64), v.astype(np.uint64))


def edge_f_coeff(wl):
    """f_coeff (N, RE): every other column holds 0, +-1, +-2, +-b/2, +-(B/2 - 1), +-B/2 in turn (shifted by the coefficient index, so that every row of the planes
    sees every edge), random values of (-B/2, B/2) between them.  +B/2 = 2^31 is left out at B = 2^32: an int32 plane cannot hold it (LF_ERR_UNSUPPORTED at ingest)"""
    B, b, N, RE = wl.B, wl.b, wl.N, wl.RE
    edges = [0, 1, -1, 2, -2, b // 2, -(b // 2), B // 2 - 1, -(B // 2 - 1), B // 2, -(B // 2)]
    if B == 1 << 32:
        edges.remove(B // 2)
    edges = np.array(edges, dtype=np.int64)
    v = (splitmix_fq(0xD16175, 0, N * RE) % np.uint64(B - 1)).astype(np.int64).reshape(N, RE) - (B // 2 - 1)
    i, c = np.meshgrid(np.arange(0, N, 2), np.arange(RE), indexing="ij")
    v[0::2] = edges[(i // 2 + c) % len(edges)]
    return residues(v, wl.P)


def oracle_parts(lfo, wl, f_coeff, mode):
    """decompose_B_vec_into_k_vec under the rule: (K, N, RE) canonical residues"""
    lfo.set_digit_mode(mode)
    try:
        return lfo.decompose(f_coeff, wl.b, wl.K, 1).reshape(wl.K, wl.N, wl.RE)
    finally:
        lfo.set_digit_mode(0)


def oracle_witness(lfo, wl, mode):
    """Witness::from_w_ccs of the workload under the rule: f_coeff (N, RE)"""
    lfo.set_digit_mode(mode)
    try:
        return lfo.Instance(wl).witness_from_w_ccs(wl.w_ccs).reshape(wl.N, wl.RE)
    finally:
        lfo.set_digit_mode(0)
