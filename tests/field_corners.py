"""Reduction-corner operands, a big-integer reference and branch predicates for the field-arithmetic tests.  TEST INFRASTRUCTURE ONLY (imported by name, like lfo.py).

Pseudo-random residues never take the rare branches of the Goldilocks reductions in latticefold_amd/csrc/lf_field.cuh: the borrow (`lo < hh`) and the
`hl == 0` case of fq_reduce128_loose, a loose result in [p, 2^64) that fq_canon must fix, either wrap of fq_from_s128.  The values below do.  Three things live here:

  * EDGE_G / EDGE_B, corner_table(), all_pairs(): the operands.
  * Ref: the operations of the kernels under test on Python ints with `%` -- independent of lf_field.cuh and of the oracle's fast reduction.
  * classes_fp() / classes_fp3(): which branches a product takes, as predicates on the operands that mirror the structure of the code without calling it
    (tests/test_field_corners_cpu.py proves with them that every GPU case reaches every corner).

The case builders at the end are shared by tests/test_field_corners_cpu.py (reference against oracle, coverage) and tests/test_gpu_field_corners.py (device
against reference), so both see the same tables.

BabyBear has a section of its own at the end: its kernels work on centred Montgomery words in [-H, H] (bb_field.cuh), so its corner grid EDGE_BW is a grid of
DEVICE words (canon() gives the residue the ABI takes), with the saturating pairs, tables of +-H, classes_bb() / classes_hl() / count_classes_dig() and the
cases of tests/test_bb_field_corners_cpu.py and tests/test_gpu_bb_field_corners.py.  EDGE_B, the canonical grid, stays for its earlier users."""
import numpy as np

from latticefold_amd.workload import RINGS, default_nonres, diag, make_workload, splitmix_fq

PG = 2**64 - 2**32 + 1
PB = 15 * 2**27 + 1
EPS = 2**32 - 1
M64 = 1 << 64
EDGE_G = [0, 1, 2, PG - 1, PG - 2, EPS, EPS + 1, EPS + 2, EPS + 3, PG - EPS, EPS - 1, (PG - 1) // 2, (PG + 1) // 2, 1 << 63, (1 << 63) + 1, 1 << 40,
          1 << 24, PG - (1 << 40), 0xFFFFFFFE00000001, 3 << 62, 0x1FFFFFFFF, PG - (1 << 24)]
# (the issue's list names p - 1, p - 2 and p - 2^32 twice -- as 2^64 - 2^32, 0xFFFFFFFEFFFFFFFF and 0xFFFFFFFE00000001: 2^32 - 2, 3 * 2^62 and p - 2^24 take the free places)
EDGE_B = [0, 1, 2, PB - 1, PB - 2, (PB - 1) // 2, (PB + 1) // 2, 1 << 15, 1 << 27, 15 << 27]
assert len(set(EDGE_G)) == 22 and all(0 <= v < PG for v in EDGE_G) and all(0 <= v < PB for v in EDGE_B)
# BabyBear: the device stores a residue x as the centred Montgomery word centre(x 2^32 mod p) in [-H, H] (latticefold_amd/csrc/bb_field.cuh), and every bound its
# kernels rely on is a bound on that word.  EDGE_BW is a grid of DEVICE WORDS; canon() maps a word to the canonical residue the ABI takes.
HB = (PB - 1) // 2
RB = (1 << 32) % PB
_RB_INV = pow(RB, PB - 2, PB)


def canon(w):
    """device word -> canonical residue: w 2^-32 mod p"""
    return w * _RB_INV % PB


def word(x):
    """canonical residue -> device word"""
    w = x * RB % PB
    return w - PB if w > HB else w


EDGE_BW = [0, 1, -1, 2, -2, HB, -HB, HB - 1, -(HB - 1), HB // 2, -(HB // 2), HB // 2 + 1, -(HB // 2 + 1), RB, -RB, 1 << 29, -(1 << 29),
           0x3B7F7F7F, -0x3B7F7F7F, 0x3B808080, -0x3B808080, 0x007F7F7F, -0x00808080, 0x7F, -0x80, 0x80, -0x81, 0x7FFF, 0x8000, -0x8000]
EDGE_BWC = [canon(w) for w in EDGE_BW]
assert len(set(EDGE_BW)) == 30 and all(-HB <= w <= HB for w in EDGE_BW) and all(word(c) == w for c, w in zip(EDGE_BWC, EDGE_BW)) and HB == 0x3C000000
FP_CLASSES = ("borrow", "hl0", "carry", "loose")
FP3_CLASSES = ("s128_up", "s128_down", "s128_loose")
CLASSES = FP_CLASSES + FP3_CLASSES


def grid(ring="goldilocks", words=False):
    """the corner operands of a ring as canonical residues; words=True (BabyBear): the device-word grid EDGE_BW through canon()"""
    if words:
        assert ring == "babybear"
        return EDGE_BWC
    return EDGE_G if ring == "goldilocks" else EDGE_B


def corner_table(seed, shape, ring="goldilocks", words=False):
    """canonical residues of the given shape: three extension-field elements in five (element e = word index // tau, chosen when (7 e + e // 8) % 5 < 3) have ALL
    their words on the grid, each picked by a SplitMix64 word -- the wraps of fq_from_s128 need whole grid operands --; the other elements are splitmix_fq words"""
    n = int(np.prod(shape))
    g = np.array(grid(ring, words), dtype=np.uint64)
    w = splitmix_fq(seed, 0, n, ring)
    pick = splitmix_fq(seed ^ 0xC0121E25, n, n, "goldilocks")
    e = np.arange(n, dtype=np.uint64) // np.uint64(RINGS[ring][2])
    edge = ((np.uint64(7) * e + e // np.uint64(8)) % np.uint64(5)) < np.uint64(3)
    out = np.where(edge, g[(pick >> np.uint64(17)) % np.uint64(len(g))], w)
    if words:
        # the top of a 64-bit column needs nine terms of one sign: a third of the grid elements are constant over their nine words, one of +-H, +-(H - 1)
        # (grid places 5..8), chosen and picked by the SplitMix64 word of the element's first word
        first = pick[::9][:(n + 8) // 9]
        big = np.repeat(g[5:9][(first >> np.uint64(23)) % np.uint64(4)], 9)[:n]
        out = np.where(edge & np.repeat((first >> np.uint64(29)) % np.uint64(3) == 0, 9)[:n], big, out)
    return out.reshape(shape)


def grid_share(a, ring="goldilocks", words=False):
    return float(np.isin(np.asarray(a, dtype=np.uint64), np.array(grid(ring, words), dtype=np.uint64)).mean())


def saturating_pairs(nu=2):
    """BabyBear, one pair (a, b) of F_{p^9} elements (canonical) per output column k = 0..8 and sign: every term of column k of a * b, as e9_mul_pre forms it
    (sum_{i<=k} a_i b_{k-i} + sum_{i>k} a_i (nu b)_{k+9-i}), is +H^2 resp. -H^2 -- a_i = +-H, b_j = H for j <= k, and for j > k the b_j whose product by nu is
    the word H (nu = 2: the word H / 2, doubled without a wrap; any other nu: canon(H) / nu)"""
    half = canon(HB // 2) if nu == 2 else canon(HB) * pow(nu, PB - 2, PB) % PB
    assert word(half * nu % PB) == HB
    out = []
    for sign in (1, -1):
        for k in range(9):
            out.append(((canon(sign * HB),) * 9, tuple(canon(HB) if j <= k else half for j in range(9))))
    return out


def all_pairs(ring="goldilocks", words=False, rotations=None, sat_nus=()):
    """(A, B): ring elements whose slot-wise products enumerate grid x grid in every pair of coordinate positions (rotation 0: a = (x, .., x), b = (y, .., y); the
    other tau - 1 rotations mix the grid over the coordinates).  The last element is padded with the first pairs.  words=True: the BabyBear device-word grid;
    sat_nus: the saturating pairs of these non-residues come first; rotations: the first so many rotations only."""
    _p, RE, tau = RINGS[ring]
    g = grid(ring, words)
    ng = len(g)
    a, b = [], []
    for nu in sat_nus:
        for x, y in saturating_pairs(nu):
            a.append(list(x)); b.append(list(y))
    for sh in range(tau if rotations is None else rotations):
        for x in range(ng):
            for y in range(ng):
                a.append([g[(x + q * sh) % ng] for q in range(tau)])
                b.append([g[(y + 5 * q * sh) % ng] for q in range(tau)])
    slots = RE // tau
    while len(a) % slots:
        a.append(a[len(a) % slots]); b.append(b[len(b) % slots])
    return np.array(a, dtype=np.uint64).reshape(-1, RE), np.array(b, dtype=np.uint64).reshape(-1, RE)


# ---- branch predicates ------------------------------------------------------------------------------------------------------
def classes_fp(a, b):
    """branches of fq_reduce128_loose on the 128-bit product a b, and whether its result needs fq_canon"""
    pr = a * b
    return _classes_lohi(pr % M64, pr >> 64)


def _s128(v):
    """fq_from_s128 on the signed value v = lo + 2^64 hi"""
    lo = v % M64
    hi = (v - lo) >> 64
    t = hi * EPS
    s = lo + t
    cls = set()
    if s >= M64:
        cls.add("s128_up")
        s = s - M64 + EPS
    elif s < 0:
        cls.add("s128_down")
        s = s + M64 - EPS
    assert 0 <= s < M64 and s % PG == v % PG
    if s >= PG:
        cls.add("s128_loose")
    return cls


def _lh(pairs):
    """(L, H) of a column sum of 64 x 64 products kept as three sums of 32 x 32 partial products with carry counters (AccP, accp_lh)"""
    s00 = s01 = s11 = 0
    for x, y in pairs:
        x0, x1, y0, y1 = x & EPS, x >> 32, y & EPS, y >> 32
        s00 += x0 * y0
        s01 += x0 * y1 + x1 * y0
        s11 += x1 * y1
    c00, s00 = s00 >> 64, s00 % M64
    c01, s01 = s01 >> 64, s01 % M64
    c11, s11 = s11 >> 64, s11 % M64
    T = (s01 >> 32) + (s11 & EPS) + c00
    U = (s11 >> 32) + c01
    return (s00 & EPS) - T - U, (s00 >> 32) + (s01 & EPS) + T - c11


def classes_fp3(a, b, nu=1 << 40):
    """nu = 2^40: the wraps of fq_from_s128 in the three linear forms of fq3_mul_2p40 / lh5_finish for ONE product; any other nu: the generic product reduces
    its five 128-bit column sums and two products by nu through fq_reduce128_loose, whose classes are returned instead"""
    cols = [[(a[i], b[k - i]) for i in range(3) if 0 <= k - i < 3] for k in range(5)]
    cls = set()
    if nu == 1 << 40:
        c = [_lh(pp) for pp in cols]
        cls |= _s128(c[0][0] - (c[3][1] << 8) + (c[0][1] << 32) + ((c[3][0] + c[3][1]) << 40))
        cls |= _s128(c[1][0] - (c[4][1] << 8) + (c[1][1] << 32) + ((c[4][0] + c[4][1]) << 40))
        cls |= _s128(c[2][0] + (c[2][1] << 32))
        return cls
    red = []
    for pp in cols:
        s = sum(x * y for x, y in pp)
        lo, hi = s % M64, (s >> 64) % M64          # (the third word is Acc.ov, folded in by a subtraction)
        cls |= _classes_lohi(lo, hi)
        if s >> 128:
            cls.add("ov")
        red.append(s % PG)
    cls |= classes_fp(red[3], nu) | classes_fp(red[4], nu)
    return cls


def _classes_lohi(lo, hi):
    """(hi:lo) -> loose residue: `lo < hh` borrows p, hl (2^32 - 1) is added without a multiply (hl == 0 is its special case), a carry out of 64 bits gives p back"""
    hh, hl = hi >> 32, hi & EPS
    cls = set()
    t0 = lo - hh
    if lo < hh:
        cls.add("borrow"); t0 += M64 - EPS
    if hl == 0:
        cls.add("hl0")
    r = t0 + hl * EPS
    if r >= M64:
        cls.add("carry"); r = r - M64 + EPS
    assert r < M64 and r % PG == (lo + (hi << 64)) % PG
    if r >= PG:
        cls.add("loose")
    return cls


def count_classes(pairs, nu=1 << 40, limit=2048, grid_only=False, distinct=False):
    """hits of each class over the first `limit` F_{p^3} operand pairs: the F_p classes over their nine coordinate products, the F_{p^3} classes over the pairs.
    grid_only: count over the pairs whose operands are grid words alone (a subset of what the kernel multiplies, so a hit there is a hit of the kernel's);
    distinct: every distinct operand pair once (tables of one value repeat the same few products thousands of times)"""
    if distinct:
        pairs = list(dict.fromkeys(pairs))
    hits = dict.fromkeys(CLASSES if nu == 1 << 40 else FP_CLASSES + ("ov",), 0)
    if grid_only:
        gs = set(EDGE_G)
        pairs = [(a, b) for a, b in pairs if gs.issuperset(a) and gs.issuperset(b) and any(a[1:]) and any(b[1:])]
    for a, b in pairs[:limit]:
        seen = set()
        for x in a:
            for y in b:
                seen |= classes_fp(x, y)
        for k in seen | classes_fp3(a, b, nu):
            hits[k] += 1
    return hits


# ---- the reference ------------------------------------------------------------------------------------------------------------
def elems(arr, ring="goldilocks"):
    """(.., RE) words -> nested lists of ring elements, each a list of 8 slot tuples of Python ints"""
    _p, RE, tau = RINGS[ring]
    a = np.asarray(arr, dtype=np.uint64)
    if a.ndim == 1:
        w = [int(v) for v in a]
        return [tuple(w[k:k + tau]) for k in range(0, RE, tau)]
    return [elems(x, ring) for x in a]


def exts(arr):
    """(n, tau) words -> list of extension-field tuples"""
    return [tuple(int(v) for v in row) for row in np.asarray(arr, dtype=np.uint64)]


def pack(e):
    """ring elements (nested lists of slot tuples) -> uint64 array (.., RE)"""
    if isinstance(e[0], tuple):
        return np.array([v for sl in e for v in sl], dtype=np.uint64)
    return np.stack([pack(x) for x in e])


class Ref:
    """F_p, F_{p^tau} = F_p[Y]/(Y^tau - nu) and the slot-wise ring (8 slots) on Python ints; `log`, when a list, receives every extension-field operand pair"""

    def __init__(self, ring="goldilocks", nu=None):
        self.ring = ring
        self.p, self.RE, self.tau = RINGS[ring]
        self.nu = default_nonres(ring) if nu is None else nu
        self.log = None
        self.one = (1,) + (0,) * (self.tau - 1)
        self.zero = (0,) * self.tau

    # F_p
    def fadd(self, a, b):
        return (a + b) % self.p

    def fsub(self, a, b):
        return (a - b) % self.p

    def fmul(self, a, b):
        return (a * b) % self.p

    # F_{p^tau}
    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def mul(self, a, b):
        if self.log is not None:
            self.log.append((a, b))
        tau = self.tau
        col = [0] * (2 * tau - 1)
        for i in range(tau):
            for j in range(tau):
                col[i + j] += a[i] * b[j]
        return tuple((col[k] + (self.nu * col[k + tau] if k + tau < 2 * tau - 1 else 0)) % self.p for k in range(tau))

    # ring elements: lists of 8 slots
    def radd(self, x, y):
        return [self.add(a, b) for a, b in zip(x, y)]

    def rsub(self, x, y):
        return [self.sub(a, b) for a, b in zip(x, y)]

    def rmul(self, x, y):
        return [self.mul(a, b) for a, b in zip(x, y)]

    def rscale(self, x, e):
        return [self.mul(a, e) for a in x]

    def rzero(self):
        return [self.zero] * (self.RE // self.tau)

    def spmv(self, rowptr, col, val, z, m):
        """mat_vec_mul on CSR: row sums of slot-wise products"""
        out = []
        for r in range(m):
            acc = self.rzero()
            for k in range(int(rowptr[r]), int(rowptr[r + 1])):
                acc = self.radd(acc, self.rmul(val[k], z[int(col[k])]))
            out.append(acc)
        return out

    def eq_table(self, pt):
        """eq[i] = prod_j (i_j ? r_j : 1 - r_j), bit j of i <-> variable j (LSB first, as k_build_eq)"""
        t = [self.one]
        for r in pt:
            om = self.sub(self.one, r)
            t = [self.mul(e, om) for e in t] + [self.mul(e, r) for e in t]
        return t

    def mle_eval(self, table, pt):
        """evaluate(): sum_i eq(pt, i) table[i], the table zero-padded to 2^nv"""
        eq = self.eq_table(pt)
        acc = self.rzero()
        for i, x in enumerate(table):
            acc = self.radd(acc, self.rscale(x, eq[i]))
        return acc

    def lincomb(self, coef, tables):
        """compute_f_0: out[x] = sum_i coef_i (.) tables_i[x]"""
        out = []
        for x in range(len(tables[0])):
            acc = self.rzero()
            for c, t in zip(coef, tables):
                acc = self.radd(acc, self.rmul(c, t[x]))
            out.append(acc)
        return out

    def horner_combine(self, tables, ch):
        """calculate_challenged_mz_mle as lfo.horner_combine states it: out = sum_i H_i, H_i: for T in reversed(group i): acc += T; acc *= ch_i"""
        ln = len(tables[0][0])
        out = []
        for x in range(ln):
            tot = self.rzero()
            for grp, c in zip(tables, ch):
                acc = self.rzero()
                for t in reversed(grp):
                    acc = self.rscale(self.radd(acc, t[x]), c)
                tot = self.radd(tot, acc)
            out.append(tot)
        return out

    def horner_pairs(self, tables, ch):
        """the products the DEVICE forms for the same sum: c_i^(j+1) T_ij[x] (k_lincomb_z with power coefficients)"""
        log, self.log = self.log, None
        pairs = []
        for grp, c in zip(tables, ch):
            pw = c
            for t in grp:
                pairs += [(sl, pw) for x in t for sl in x]
                pw = self.mul(pw, c)
        self.log = log
        return pairs

    def fix(self, table, r):
        """fix_variables(&[r]): new[j] = old[2j] + r (old[2j+1] - old[2j])"""
        return [self.radd(table[2 * j], self.rscale(self.rsub(table[2 * j + 1], table[2 * j]), r)) for j in range(len(table) // 2)]

    def lin_rounds(self, tables, beta, S_off, S_idx, c, d, challenges):
        """the round messages of the linearization sumcheck: round k's message at X = 0 .. d+1 is the sum over the remaining cube of
        eq(beta, .) sum_i c_i prod_{j in S_i} M_j(.), variable k (the LSB of what remains) replaced by X; challenges[k] fixes it before round k+1"""
        tabs = [list(t) for t in tables]
        eq = [[e] * (self.RE // self.tau) for e in self.eq_table(beta)]
        nv = len(beta)
        msgs = []
        for rnd in range(nv):
            if rnd:
                r = challenges[rnd - 1]
                tabs = [self.fix(t, r) for t in tabs]
                eq = self.fix(eq, r)
            msg = [self.rzero() for _ in range(d + 2)]
            for b in range(len(eq) // 2):
                lo = [t[2 * b] for t in tabs] + [eq[2 * b]]
                step = [self.rsub(t[2 * b + 1], t[2 * b]) for t in tabs] + [self.rsub(eq[2 * b + 1], eq[2 * b])]
                vals = lo
                for X in range(d + 2):
                    if X:
                        vals = [self.radd(v, s) for v, s in zip(vals, step)]
                    res = self.rzero()
                    for i in range(len(S_off) - 1):
                        term = c[i]
                        for k in range(int(S_off[i]), int(S_off[i + 1])):
                            term = self.rmul(term, vals[int(S_idx[k])])
                        res = self.radd(res, term)
                    msg[X] = self.radd(msg[X], self.rmul(res, vals[-1]))
            msgs.append(msg)
        return msgs


# ---- the products the device forms (the coverage condition counts these, not the reference's) --------------------------------------------
def _logged_eq(ref, pt):
    keep, ref.log = ref.log, []
    t = ref.eq_table(pt)
    pairs, ref.log = ref.log, keep
    return t, pairs


def eq_device_pairs(ref, pt):
    """(eq table, operand pairs) of build_eq as the device forms it: below 6 variables every entry is the running product of its nv factors (k_build_eq: the
    distinct (prefix, factor) pairs are those of the doubling recursion); from 6 on two half tables are built that way and multiplied entry by entry (k_eq_outer).
    BabyBear (the ring is the reference's): lfbb::k_build_eq forms the running product at every size, the factor being the pre-multiplied operand"""
    nv = len(pt)
    if nv < 6 or ref.ring == "babybear":
        return _logged_eq(ref, pt)
    hl = nv // 2
    lo, p1 = _logged_eq(ref, pt[:hl])
    hi, p2 = _logged_eq(ref, pt[hl:])
    keep, ref.log = ref.log, None
    eq = [ref.mul(a, b) for b in hi for a in lo]
    ref.log = keep
    return eq, p1 + p2 + [(a, b) for b in hi for a in lo]


def mle_device_pairs(table, eq):
    """evaluate_mles: one product per entry and slot with the eq entry (k_dot_eq / k_dot_batch: acc += x e)"""
    return [(sl, eq[i]) for i, x in enumerate(table) for sl in x]


def fold_round1_pairs(ref, wl, tabs, mu, npairs=4):
    """every F_{p^3} product round 1 of the folding sumcheck forms for its first `npairs` pairs, all slots, from tables laid out as MLSumcheckFold takes them
    (eqL, G1, eqR, G2, eqB, then f-hat_kd with weight mu_k^(d+1)): the three products of (e0 + X de)(g0 + X dg) per half (lf_rounds.hip: fold_g13), then
      b = 2 (k_fold_round): f0^2, df^2, mu f0, mu df, the four lazy products (mu f0) f0^2 .. (mu df) df^2 per table, Q(X) eqB(X) at X = 0..4;
      b > 2 (lf_sb.hip: k_sb_round): at X = 0..2b  f^2, f prod_j (f^2 - j^2), mu times that per table, and S(X) eqB(X).
    The eq tables themselves come from the caller (the GPU test builds them on the host), so their products are not counted."""
    T = [elems(t[:2 * npairs], ref.ring) for t in tabs]
    mus = exts(mu)
    b, nkd = wl.b, 2 * wl.K * wl.tau
    keep, ref.log = ref.log, None
    mupow = []
    for m in mus:
        pw = m
        for _ in range(wl.tau):
            mupow.append(pw)
            pw = ref.mul(pw, m)
    ref.log = []
    small = lambda k: (k % ref.p, 0, 0)
    for p in range(npairs):
        for sl in range(ref.RE // ref.tau):
            at = lambda j, i: T[j][2 * p + i][sl]
            for e, g in ((0, 1), (2, 3)):
                ref.mul(at(e, 0), at(g, 0))
                ref.mul(ref.sub(at(e, 1), at(e, 0)), ref.sub(at(g, 1), at(g, 0)))
                ref.mul(at(e, 1), at(g, 1))
            e0, es = at(4, 0), ref.sub(at(4, 1), at(4, 0))
            npt = 5 if b == 2 else 2 * b + 1
            S = [ref.zero] * npt
            if b == 2:
                A = [ref.zero] * 4
                sp = sq = ref.zero
                for kd in range(nkd):
                    f0, m = at(5 + kd, 0), mupow[kd]
                    df = ref.sub(at(5 + kd, 1), f0)
                    f0s, dfs, pp, qq = ref.mul(f0, f0), ref.mul(df, df), ref.mul(m, f0), ref.mul(m, df)
                    for i, (x, y) in enumerate(((pp, f0s), (qq, f0s), (pp, dfs), (qq, dfs))):
                        A[i] = ref.add(A[i], ref.mul(x, y))
                    sp, sq = ref.add(sp, pp), ref.add(sq, qq)
                three = lambda x: ref.add(ref.add(x, x), x)
                Q = [ref.sub(A[0], sp), ref.sub(three(A[1]), sq), three(A[2]), A[3]]
                for X in range(npt):
                    v = ref.zero
                    for c in reversed(Q):
                        v = ref.add(tuple(w * X % ref.p for w in v), c)
                    S[X] = v
            else:
                for kd in range(nkd):
                    f, m = at(5 + kd, 0), mupow[kd]
                    df = ref.sub(at(5 + kd, 1), f)
                    for X in range(npt):
                        f2 = ref.mul(f, f)
                        prod = f
                        for j in range(1, b):
                            prod = ref.mul(prod, ref.sub(f2, small(j * j)))
                        S[X] = ref.add(S[X], ref.mul(m, prod))
                        f = ref.add(f, df)
            e = e0
            for X in range(npt):
                ref.mul(S[X], e)
                e = ref.add(e, es)
    pairs, ref.log = ref.log, keep
    return pairs


# ---- cases shared by the CPU and the GPU tests ----------------------------------------------------------------------------------
def other_nonresidue():
    """(nu, y tables) of F_{p^3} = F_p[Y]/(Y^3 - w^5), w = 2^40: the generic-nu instantiation of every Goldilocks kernel (as test_fold_step_with_another_nonresidue)"""
    w = 1 << 40
    y2 = np.zeros((8, 3), dtype=np.uint64)
    for k, e in enumerate([1, 5, 7, 11, 13, 17, 19, 23]):
        g = 1 if e % 3 == 2 else 2
        y2[k, g] = pow(w, ((e - 5 * g) % 24) // 3, PG)
    return pow(w, 5, PG), y2.reshape(-1)


def point(kind, nv, ring="goldilocks", shift=0, words=False):
    """nv extension-field coordinates: "grid" walks the grid, "pm1" / "half" are all p - 1 / all (p + 1) / 2, "bits" a 0 / 1 point; BabyBear also "wmax" /
    "wmin": every coordinate the device word H / -H"""
    p, _RE, tau = RINGS[ring]
    g = grid(ring, words)
    if kind == "grid":
        return np.array([[g[(shift + 5 * j + 3 * q) % len(g)] for q in range(tau)] for j in range(nv)], dtype=np.uint64)
    if kind in ("wmax", "wmin"):
        return np.full((nv, tau), canon(HB if kind == "wmax" else -HB), dtype=np.uint64)
    if kind == "pm1":
        return np.full((nv, tau), p - 1, dtype=np.uint64)
    if kind == "half":
        return np.full((nv, tau), (p + 1) // 2, dtype=np.uint64)
    assert kind == "bits"
    pt = np.zeros((nv, tau), dtype=np.uint64)
    pt[:, 0] = (np.arange(nv) + shift) % 2
    return pt


def challenges(n, ring="goldilocks", words=False):
    """n round challenges from the grid; the first three put 0, 1 and p - 1 into every coordinate (words=True: the canonical values of the device words
    0, R and -R, which are the same three residues)"""
    p, _RE, tau = RINGS[ring]
    g = grid(ring, words)
    sp = [canon(0), canon(RB), canon(-RB)] if words else [0, 1, p - 1]
    out = [[sp[(k + q) % 3] for q in range(tau)] for k in range(3)]
    out += [[g[(7 * k + 4 * q + 1) % len(g)] for q in range(tau)] for k in range(3, n)]
    return np.array(out[:n], dtype=np.uint64)


def table(kind, seed, shape, ring="goldilocks", words=False):
    """"corner": corner_table; "pm1": every word p - 1; BabyBear device words: "wmax" / "wmin" every word H / -H, "wsat" / "wsatb" the two sides of the
    saturating pattern (wsat_table)"""
    if kind == "corner":
        return corner_table(seed, shape, ring, words)
    if kind in ("wmax", "wmin"):
        return np.full(shape, canon(HB if kind == "wmax" else -HB), dtype=np.uint64)
    if kind in ("wsat", "wsatb"):
        return wsat_table(shape, "a" if kind == "wsat" else "b")
    return np.full(shape, RINGS[ring][0] - 1, dtype=np.uint64)


def wsat_table(shape, role, nu=2):
    """the saturating pairs tiled over a BabyBear table of shape (.., rows, 72): role "a" -- every word of row x is (-1)^x H; role "b" -- slot sl of every
    element holds the right operand of column k = 8 - sl.  A slot-wise product of an "a" element by a "b" element has column k at (-1)^x 9 H^2, and a sum of
    such products over tables (lincomb) grows with one sign per row."""
    assert shape[-1] == 72
    sat = saturating_pairs(nu)
    rows = shape[-2] if len(shape) > 1 else 1
    if role == "a":
        one = np.array([[canon(HB if x % 2 == 0 else -HB)] * 72 for x in range(rows)], dtype=np.uint64)
    else:
        one = np.tile(np.array([v for sl in range(8) for v in sat[8 - sl][1]], dtype=np.uint64), (rows, 1))
    return np.broadcast_to(one if len(shape) > 1 else one[0], shape).copy()


PRODUCT_KINDS = ("one", "two", "rows")


def products_case(kind, ring="goldilocks"):
    """(workload, z): matrix 0 of a T10 / B6-shaped workload carries the all_pairs() left operands, z the right ones -- "one": one entry per row (k_spmv);
    "two": two entries in every other row, 1.5 per row on average, still k_spmv; "rows": three per row, the general layout (k_spmv_rows on Goldilocks)"""
    wl = make_workload("T10" if ring == "goldilocks" else "B8")
    A, B = all_pairs(ring)
    ne, rows = len(A), min(wl.n, wl.m)
    assert ne <= rows
    z = corner_table(0x2B, (wl.n, wl.RE), ring)
    z[:ne] = B
    per = {"one": lambda r: 1, "two": lambda r: 2 - (r & 1), "rows": lambda r: 3}[kind]
    cnt = np.array([per(r) if r < rows else 0 for r in range(wl.m)], dtype=np.uint32)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    nnz = int(rp[-1])
    col = (np.arange(nnz, dtype=np.uint32) % np.uint32(ne)).astype(np.uint32)
    wl.rowptr[0], wl.col[0], wl.val[0] = rp, col, np.ascontiguousarray(A[col])
    return wl, z


EQ_NVS = (1, 5, 6, 7, 8)
EQ_POINTS = ("grid", "pm1", "half", "bits")


def mle_tables(nv, ln, ring="goldilocks"):
    return np.stack([table("corner", 0xE0 + nv, (ln, RINGS[ring][1]), ring), table("pm1", 0, (ln, RINGS[ring][1]), ring)])


COMBINE_CASES = ((4, 67), (8, 259))      # (K, table length): 2K terms / 2K groups of t = 3, one and two blocks of 256 entries


def lincomb_case(K, ln, ring="goldilocks"):
    RE = RINGS[ring][1]
    coef = corner_table(0x1C + K, (2 * K, RE), ring)
    coef[0] = RINGS[ring][0] - 1
    return coef, corner_table(0x1D + K, (2 * K, ln, RE), ring)


def horner_case(K, ln, ring="goldilocks"):
    _p, RE, tau = RINGS[ring]
    return corner_table(0x40 + K, (2 * K, 3, ln, RE), ring), point("grid", 2 * K, ring, shift=K)


LIN_CASES = (("r1cs", "corner"), ("r1cs", "pm1"), ("deg3", "corner"), ("deg3", "pm1"))


def lin_case(ccs, kind):
    """(workload, tables [t][m], beta, challenges) of a linearization sumcheck on T8"""
    wl = make_workload("T8", ccs=ccs)
    return wl, table(kind, 0x51 + wl.t, (wl.t, wl.m, wl.RE)), point("grid", wl.s, shift=2), challenges(wl.s)


def lin_witness_case(ccs):
    """T8 with a witness drawn from the grid; the last matrix becomes diag(z^(d-1)), so that the system stays satisfied (M_0 = M_1 = I: the tables M_j z of the
    linearization are the grid witness itself and its slot-wise powers; its last quarter is p - 1 in every word)"""
    from latticefold_amd.workload import ring_mul_ntt
    wl = make_workload("T8", ccs=ccs)
    wl.w_ccs = corner_table(0x77, (wl.wit_len, wl.RE))
    wl.w_ccs[-(wl.wit_len // 4):] = PG - 1           # and a run of p - 1 at the end: the largest lazy sums of the split-eq and tail kernels
    z = wl.z()[:min(wl.n, wl.m)]
    zp = z
    for _ in range(wl.d - 2):
        zp = ring_mul_ntt(zp, z)
    wl.val[wl.t - 1] = np.ascontiguousarray(zp)
    return wl


FOLD_CASES = (("T8", "corner"), ("T8", "pm1"), ("T8b4", "corner"), ("T8b4", "pm1"))


def fold_case(name, kind):
    """(workload, tables [5 + 2K tau][m], mu [2K]) laid out as MLSumcheckFold takes them: the three eq tables (slot-constant) are left to the caller, who builds
    them from fold_eq_points() with the reference / the oracle"""
    wl = make_workload(name)
    nt = 5 + 2 * wl.K * wl.tau
    return wl, table(kind, 0xF0 + wl.b, (nt, wl.m, wl.RE)), point("grid", 2 * wl.K, shift=wl.b)


def fold_eq_points(wl, kind="corner"):
    """the points of eqL, eqR, eqB.  With tables of p - 1 alone the only products of two whole grid operands that a round forms are f-hat^2, mu f-hat (b = 2
    only: for b > 2 mu multiplies the norm polynomial's value) and eq x G: there eqR's point is one grid coordinate followed by zeros, so that its two
    non-zero entries r_0 and 1 - r_0 are grid operands too and meet G = (p-1, p-1, p-1) -- that product takes both wraps of fq_from_s128"""
    pr = point("half", wl.s)
    if kind == "pm1":
        pr = np.zeros((wl.s, wl.tau), dtype=np.uint64)
        pr[0] = point("grid", 1, shift=7)[0]
    return [point("grid", wl.s, shift=1), pr, point("grid", wl.s, shift=9)]


CRT_ROWS = ("pm1", "halfm", "halfp", "corner")


def crt_rows(kind, count):
    if kind == "corner":
        return corner_table(0xC27 + count, (count, 24))
    return np.full((count, 24), {"pm1": PG - 1, "halfm": (PG - 1) // 2, "halfp": (PG + 1) // 2}[kind], dtype=np.uint64)


def crt_matrices():
    """(F, I): crt and icrt as 24 x 24 matrices of Python ints, out[i] = sum_c M[i][c] x[c].  Both maps are F_p-linear, so the matrices are the oracle's images of
    the unit vectors (products by 0 and 1 only); the CPU test checks F I = 1 on big integers and F x, I x against the oracle on every row the GPU test feeds"""
    import lfo
    e = np.eye(24, dtype=np.uint64)
    return tuple([[int(img[c][i]) for c in range(24)] for i in range(24)] for img in (lfo.crt(e), lfo.icrt(e)))


def matvec(M, rows):
    return np.array([[sum(m * int(v) for m, v in zip(Mi, r)) % PG for Mi in M] for r in rows], dtype=np.uint64)


def dense_rows_classes(M, rows):
    """k_icrt_dense: every output word is a sum of 24 products in one Acc, reduced once -- the four classes of fq_reduce128_loose on the low 128 bits of the sum,
    and "ov": the sum reached 2^128 (Acc.ov != 0)"""
    hits = dict.fromkeys(FP_CLASSES + ("ov",), 0)
    for r in rows:
        for Mi in M:
            s = sum(m * int(v) for m, v in zip(Mi, r))
            for k in _classes_lohi(s % M64, (s >> 64) % M64) | ({"ov"} if s >> 128 else set()):
                hits[k] += 1
    return hits


def embed(pt, ring="goldilocks"):
    """extension-field coordinates -> diagonal ring elements (every slot the same), as the oracle takes points"""
    return np.tile(np.asarray(pt, dtype=np.uint64), (1, RINGS[ring][1] // RINGS[ring][2]))


# ==== BabyBear: predicates on the device word, device operand pairs and the cases shared by tests/test_bb_field_corners_cpu.py and tests/test_gpu_bb_field_corners.py ====
# bb_field.cuh multiplies centred Montgomery words: nine products of one column are added in a signed 64-bit register (|T| <= 9 H^2 < 2^63) and reduced once by
# mred, which first centres the high half of T (it exceeds H only when |T| > H 2^32, about half of the register's range) and centres again after subtracting
# the Montgomery quotient.  The classes below name those branches; they are conditions on the operands' DEVICE words, computed here from the canonical
# residues through word().
BB_MUL_CLASSES = ("pre_up", "pre_down", "post_up", "post_down", "col_top", "canon_neg")
BB_NU2_CLASSES = BB_MUL_CLASSES + ("dbl_wrap",)
BB_HL_CLASSES = ("hl_a2_pos", "hl_a2_neg", "hl_carry1")
BB_DIG_CLASSES = tuple(f"dig_m128[{u}]" for u in range(3)) + tuple(f"dig_127[{u}]" for u in range(3)) + ("dig_carry",)
PINV_B = pow(PB, -1, 1 << 32)
COL_MAX = 9 * HB * HB
assert PINV_B == 0x88000001 and COL_MAX < 1 << 63


def _s32(v):
    v &= EPS
    return v - (1 << 32) if v >> 31 else v


def _mred_classes(T):
    """(classes, result word) of the Montgomery reduction of one signed 64-bit column T: the branches of mred, and the largest columns"""
    assert abs(T) <= COL_MAX
    cls = set()
    if 10 * abs(T) > 9 << 63:
        cls.add("col_top")
    thi, tlo = T >> 32, T & EPS
    q = (_s32(tlo * PINV_B) * PB) >> 32
    if thi > HB:
        cls.add("pre_up"); thi -= PB
    elif thi < -HB:
        cls.add("pre_down"); thi += PB
    r = thi - q
    assert abs(thi) <= HB and -(1 << 31) <= r < (1 << 31)
    if r > HB:
        cls.add("post_up"); r -= PB
    elif r < -HB:
        cls.add("post_down"); r += PB
    assert abs(r) <= HB and (r * (1 << 32) - T) % PB == 0
    return cls, r


def bb_columns(a, b, nu=2):
    """(classes of forming nu b, the nine un-reduced columns T_k) of the F_{p^9} product a b with b the pre-multiplied operand, as e9_mul_pre / e9_mul_cols
    form them: T_k = sum_{i<=k} a_i b_{k-i} + sum_{i>k} a_i (nu b)_{k+9-i} on device words.  nu = 2: the doubling of e9_times_nu_t<true>, whose centre() wraps
    when |2 b_j| > H; any other nu: a Montgomery product per word (its mred classes are returned)"""
    aw, bw = [word(x) for x in a], [word(x) for x in b]
    cls = set()
    if nu == 2:
        bn = []
        for w in bw:
            d = 2 * w
            if abs(d) > HB:
                cls.add("dbl_wrap")
            bn.append(d - PB if d > HB else d + PB if d < -HB else d)
    else:
        nw = word(nu % PB)
        bn = []
        for w in bw:
            c, r = _mred_classes(w * nw)
            cls |= c
            bn.append(r)
    assert all(canon(x) == canon(w) * nu % PB for x, w in zip(bn, bw))
    return cls, [sum(aw[i] * (bw[k - i] if i <= k else bn[k + 9 - i]) for i in range(9)) for k in range(9)]


def classes_bb(a, b, nu=2):
    """the classes one F_{p^9} product a b reaches on the device (b the pre-multiplied operand); canon_neg: to_canon of a result word adds p"""
    cls, cols = bb_columns(a, b, nu)
    for T in cols:
        c, r = _mred_classes(T)
        cls |= c
        if r < 0:
            cls.add("canon_neg")
    return cls


def count_classes_bb(pairs, nu=2, limit=None, distinct=True, only=None):
    """hits of each class over F_{p^9} operand pairs (a, b) as the DEVICE forms them; only: a set of elements -- count the pairs whose operands both lie in it"""
    if distinct:
        pairs = list(dict.fromkeys(pairs))
    if only is not None:
        pairs = [(a, b) for a, b in pairs if a in only and b in only]
    hits = dict.fromkeys(BB_NU2_CLASSES if nu == 2 else BB_MUL_CLASSES, 0)
    for a, b in pairs[:limit]:
        for k in classes_bb(a, b, nu):
            hits[k] += 1
    return hits


def classes_hl(cols):
    """a lazy sum of un-reduced columns in the 96-bit accumulator HL (bb_kernels_dev.cuh: hl_add, hl_finish): hl_carry1 -- an addition carries out of the low
    word; hl_a2_pos / hl_a2_neg -- the total reaches 2^64 / falls below -2^64, so that hl_finish sees a top word other than 0 and -1"""
    cls, acc = set(), 0
    for T in cols:
        if (acc & EPS) + (T & EPS) > EPS:
            cls.add("hl_carry1")
        acc = (acc + T) % (1 << 96)
    V = sum(cols)
    assert abs(V) < 1 << 95
    if V >= 1 << 64:
        cls.add("hl_a2_pos")
    if V < -(1 << 64):
        cls.add("hl_a2_neg")
    return cls


def count_classes_hl(sums, nu=2):
    """sums: per output element the list of (a, b) whose products one accumulator adds (b pre-multiplied) -> hits of the HL classes over all nine columns"""
    hits = dict.fromkeys(BB_HL_CLASSES, 0)
    for terms in sums:
        cols = [bb_columns(a, b, nu)[1] for a, b in terms]
        for k in range(9):
            for c in classes_hl([t[k] for t in cols]):
                hits[c] += 1
    return hits


def digits_bb(w):
    """the four balanced base-256 digits of a device word (lf_i8_mma.cuh: balanced_bytes) and, per digit, whether balancing it carried into the next"""
    d, carry = [], []
    for _ in range(4):
        byte = w % 256
        r = byte - 256 if byte >= 128 else byte
        d.append(r); carry.append(byte >= 128)
        w = (w - r) >> 8
    assert w == 0
    return d, carry


def count_classes_dig(values):
    hits = dict.fromkeys(BB_DIG_CLASSES, 0)
    for x in values:
        d, carry = digits_bb(word(int(x)))
        for u in range(3):
            hits[f"dig_m128[{u}]"] += d[u] == -128
            hits[f"dig_127[{u}]"] += d[u] == 127
        hits["dig_carry"] += any(carry[:3])
    return hits


def bbdot_guard(n):
    """the exactness guard of launch_dot_batch_i8 restated (lf_dot_i8.cuh: DotPlan::make with the 12 chunks of bb_dot_i8.hip refuses `steps_per_chunk >= 2048`): a wave adds steps_per_chunk * 64
    digit products of at most 2^14 into one int32"""
    cd = lambda a, b: (a + b - 1) // b
    nsteps = cd(n, 64)
    want = min(12, nsteps)
    chunks = cd(nsteps, cd(nsteps, want))
    return -1 if cd(nsteps, chunks) >= 2048 else 0


def other_nonresidue_bb():
    """(zeta, y tables) of F_{p^9} = F_p[Y]/(Y^9 - zeta), zeta a primitive 24th root of unity: the generic-nu instantiation of the BabyBear kernels (the ring of
    test_fold_step_with_another_nonresidue)"""
    g0 = 2
    while True:
        zeta = pow(g0, (PB - 1) // 24, PB)
        if pow(zeta, 12, PB) != 1 and pow(zeta, 8, PB) != 1:
            break
        g0 += 1
    y2 = np.zeros((8, 9), dtype=np.uint64)
    for k, e in enumerate([1, 5, 7, 11, 13, 17, 19, 23]):
        g = e % 3
        a = next(t for t in range(24) if (9 * t) % 24 == (e - g) % 24)
        y2[k, g] = pow(zeta, a, PB)
    return zeta, y2.reshape(-1)


BB = "babybear"
BB_ROTATIONS = 4      # B10 holds 514 elements: 36 saturating pairs + 4 rotations of 30 x 30 grid pairs are 455 (rotation 0 alone puts every pair into every pair of positions)


def products_case_bb(kind):
    """products_case on B10 with the word-grid pairs behind the saturating pairs of nu = 2 and of the generic nu"""
    wl = make_workload("B10")
    A, B = all_pairs(BB, words=True, rotations=BB_ROTATIONS, sat_nus=(2, other_nonresidue_bb()[0]))
    ne, rows = len(A), min(wl.n, wl.m)
    assert ne <= rows
    z = corner_table(0x2B, (wl.n, wl.RE), BB, words=True)
    z[:ne] = B
    per = {"one": lambda r: 1, "two": lambda r: 2 - (r & 1), "rows": lambda r: 3}[kind]
    cnt = np.array([per(r) if r < rows else 0 for r in range(wl.m)], dtype=np.uint32)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    col = (np.arange(int(rp[-1]), dtype=np.uint32) % np.uint32(ne)).astype(np.uint32)
    wl.rowptr[0], wl.col[0], wl.val[0] = rp, col, np.ascontiguousarray(A[col])
    return wl, z


EQ_POINTS_BB = ("grid", "wmax", "wmin", "bits")


def mle_tables_bb(nv, ln):
    return np.stack([table("corner", 0xE0 + nv, (ln, 72), BB, words=True), table("wmax", 0, (ln, 72), BB)])


COMBINE_KINDS_BB = ("corner", "wmax", "wsat")


def lincomb_case_bb(K, ln, kind):
    """(coef [2K], tables [2K][ln]).  The device multiplies table element (a) by coefficient (b, pre-multiplied by nu) and adds the 2K products of an output
    un-reduced: "wsat" tables are (-1)^x H in row x and the coefficients the right operands of the saturating pairs, so the sums of 2K = 8 / 16 columns of
    +-9 H^2 pass 2^64 in both directions; "wmax": every word H on both sides"""
    if kind == "corner":
        coef = corner_table(0x1C + K, (2 * K, 72), BB, words=True)
        coef[0] = canon(HB)
        return coef, corner_table(0x1D + K, (2 * K, ln, 72), BB, words=True)
    if kind == "wmax":
        return table("wmax", 0, (2 * K, 72), BB), table("wmax", 0, (2 * K, ln, 72), BB)
    return table("wsatb", 0, (2 * K, 72), BB), table("wsat", 0, (2 * K, ln, 72), BB)


def lincomb_device_sums(coef, tables, rows=None):
    """per output (row, slot) the (table element, coefficient) pairs k_lincomb_z adds in one accumulator"""
    cf, tb = elems(coef, BB), elems(tables, BB)
    return [[(tb[i][x][sl], cf[i][sl]) for i in range(len(cf))] for x in range(len(tb[0]) if rows is None else rows) for sl in range(8)]


def horner_case_bb(K, ln, kind):
    """(tables [2K][3][ln], challenges [2K]); "wmax" / "wsat": every challenge coordinate the word H (its powers are generic), tables H resp. (-1)^x H"""
    if kind == "corner":
        return corner_table(0x40 + K, (2 * K, 3, ln, 72), BB, words=True), point("grid", 2 * K, BB, shift=K, words=True)
    return table(kind, 0, (2 * K, 3, ln, 72), BB), point("wmax", 2 * K, BB)


def horner_device_sums(ref, tables, ch, rows=None):
    """per output (row, slot) the (table element, power of the challenge) pairs the device adds in one accumulator (k_lincomb_z with power coefficients)"""
    keep, ref.log = ref.log, None
    tb, cs = elems(tables, BB), exts(ch)
    pw = []
    for c in cs:
        p = c
        for _ in range(len(tb[0])):
            pw.append(p)
            p = ref.mul(p, c)
    ref.log = keep
    flat = [t for grp in tb for t in grp]
    return [[(flat[i][x][sl], pw[i]) for i in range(len(flat))] for x in range(len(flat[0]) if rows is None else rows) for sl in range(8)]


LIN_CASES_BB = tuple((c, k) for c in ("r1cs", "deg3") for k in ("corner", "wmax", "wsat"))


def lin_case_bb(ccs, kind):
    """(workload, tables [t][m], beta, challenges) of a linearization sumcheck on B6.  "wsat": table 0 is the left side of the saturating pattern, table 1 the
    right side (the first product of the first term is M_0 M_1, M_1 pre-multiplied), the others H"""
    wl = make_workload("B6", ccs=ccs)
    shape = (wl.t, wl.m, wl.RE)
    if kind == "wsat":
        tabs = table("wmax", 0, shape, BB)
        tabs[0], tabs[1] = table("wsat", 0, shape[1:], BB), table("wsatb", 0, shape[1:], BB)
    else:
        tabs = table(kind, 0x51 + wl.t, shape, BB, words=True)
    return wl, tabs, point("grid", wl.s, BB, shift=2, words=True), challenges(wl.s, BB, words=True)


FOLD_CASES_BB = (("B6", "corner"), ("B6", "wmax"), ("B8", "corner"), ("B8", "wmax"))


def fold_case_bb(name, kind):
    """(workload, tables [5 + 2K tau][m], mu [2K]) as MLSumcheckFold takes them; the eq tables are built by the caller from fold_eq_points_bb()"""
    wl = make_workload(name)
    nt = 5 + 2 * wl.K * wl.tau
    mu = point("grid", 2 * wl.K, BB, shift=wl.b, words=True)
    if kind == "wmax":
        mu[0] = canon(-HB)          # tables of +H alone square to +9 H^2: mu_0 f-hat is the column of -9 H^2
    return wl, table(kind, 0xF0 + wl.b, (nt, wl.m, wl.RE), BB, words=True), mu


def fold_eq_points_bb(wl, kind):
    """the points of eqL, eqR, eqB from the word grid; with "wmax" tables eqR's point is one grid coordinate followed by zeros, so that its two non-zero
    entries r_0 and 1 - r_0 are whole grid operands against G (the construction of fold_eq_points)"""
    pr = point("wmin", wl.s, BB)
    if kind == "wmax":
        pr = np.zeros((wl.s, wl.tau), dtype=np.uint64)
        pr[0] = point("grid", 1, BB, shift=5, words=True)[0]
    return [point("grid", wl.s, BB, shift=1, words=True), pr, point("grid", wl.s, BB, shift=9, words=True)]


CRT_ROWS_BB = ("wmax", "wmin", "wsat", "corner")
CRT_COUNTS_BB = (1, 63, 65, 257)


def crt_matrices_bb():
    """(F, I): crt and icrt of the BabyBear ring as 72 x 72 matrices of Python ints, the oracle's images of the unit vectors (as crt_matrices)"""
    import lfo_bb
    e = np.eye(72, dtype=np.uint64)
    return tuple([[int(img[c][i]) for c in range(72)] for i in range(72)] for img in (lfo_bb.crt(e), lfo_bb.icrt(e)))


def matvec_bb(M, rows):
    Mn = np.array(M, dtype=object)
    return np.array([[int(v) % PB for v in Mn.dot(np.array([int(v) for v in r], dtype=object))] for r in rows], dtype=np.uint64)


def crt_rows_bb(kind, count, I):
    """"wsat": row r takes, for output word i = r % 72 of the dense inverse map, x_c = sign(word(I[i][c])) H -- every product of that output has the sign of
    its matrix entry squared away, so each nine-term group of icrt_dense_elem is as large as the matrix allows"""
    if kind == "corner":
        return corner_table(0xC27 + count, (count, 72), BB, words=True)
    if kind in ("wmax", "wmin"):
        return table(kind, 0, (count, 72), BB)
    return np.array([[canon(HB if word(I[r % 72][c]) >= 0 else -HB) for c in range(72)] for r in range(count)], dtype=np.uint64)


def icrt_group_classes(I, rows):
    """k_icrt_dense: every output word adds eight mred results of nine-term groups sum_c M[i][9g + c] x[9g + c] -- the mred classes over all groups, and the
    largest |T| / 2^63 seen"""
    Iw = [[word(v) for v in r] for r in I]
    hits, top = dict.fromkeys(BB_MUL_CLASSES[:5], 0), 0
    for r in rows:
        xw = [word(int(v)) for v in r]
        for Mi in Iw:
            for g in range(8):
                T = sum(Mi[9 * g + c] * xw[9 * g + c] for c in range(9))
                top = max(top, abs(T))
                for k in _mred_classes(T)[0]:
                    hits[k] += 1
    return hits, top / 2.0**63


SELFTEST_PAIRS_BB = 9 * 30 * 30 + 36          # operand pairs of BbCtx::selftest_field that come from the grid: every rotation, then the saturating pairs of 2 and of the context's nu


# ---- the int8 inner products through the decomposition prover -------------------------------------------------------------------------------------------
DOT_SHAPES_BB = (("B8", 63), ("B8", 1))        # (workload, public inputs): n = wit_len + l + 1 = 192 columns (three steps of 64) and 130 (no multiple of 64)
DOT_I0 = 5                                     # the row of every matrix made dense; r = its bits


def dot_y_words(n):
    """n ring elements of device words for the dense row: every digit-boundary word, +-H, and runs of -0x3B808080 (digits -128, -128, -128, -59)"""
    t = corner_table(0xD07, (n, 72), BB, words=True)
    t[3:11] = canon(-0x3B808080)
    t[20:24] = canon(0x3B7F7F7F)
    t[30] = canon(HB); t[31] = canon(-HB)
    return t


def dot_case_bb(name, l):
    """a workload whose matrices have row DOT_I0 dense over all n columns with dot_y_words, and the 0 / 1 point r of that row: eq(r) is the row's indicator, so
    M_j^T eq(r) -- the Y operand of k_dot_pack_y / k_bbdot_i8 -- is that row"""
    wl = make_workload(name, l=l)
    for j in range(wl.t):
        rp, col, val = (np.asarray(a) for a in (wl.rowptr[j], wl.col[j], wl.val[j]))
        a, b = int(rp[DOT_I0]), int(rp[DOT_I0 + 1])
        dense = np.roll(dot_y_words(wl.n), 7 * j, axis=0)
        wl.col[j] = np.concatenate([col[:a], np.arange(wl.n, dtype=np.uint32), col[b:]]).astype(np.uint32)
        wl.val[j] = np.ascontiguousarray(np.concatenate([val[:a], dense, val[b:]]))
        rp = rp.astype(np.int64)
        rp[DOT_I0 + 1:] += wl.n - (b - a)
        wl.rowptr[j] = rp.astype(np.uint32)
    r = np.zeros((wl.s, wl.RE), dtype=np.uint64)
    for i in range(wl.s):
        r[i, ::wl.tau] = (DOT_I0 >> i) & 1
    return wl, r


CE_WORDS_BB = (0x3B7F7F7F, -0x3B808080, 0x3B808080, -0x00808080, 0x007F7F7F, HB)


def ce_point(wl, w):
    """r = (x, 0, .., 0) with x = canon(w) in every coordinate: eq(r) has the two non-zero entries 1 - x and x, corner words that k_bbce_i8 cuts into digits"""
    r = np.zeros((wl.s, wl.RE), dtype=np.uint64)
    r[0] = np.tile(np.full(wl.tau, canon(w), dtype=np.uint64), 8)
    return r
