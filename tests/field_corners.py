"""Reduction-corner operands, a big-integer reference and branch predicates for the field-arithmetic tests.  TEST INFRASTRUCTURE ONLY (imported by name, like lfo.py).

Pseudo-random residues never take the rare branches of the Goldilocks reductions in latticefold_amd/csrc/lf_field.cuh: the borrow (`lo < hh`) and the
`hl == 0` case of fq_reduce128_loose, a loose result in [p, 2^64) that fq_canon must fix, either wrap of fq_from_s128.  The values below do.  Three things live here:

  * EDGE_G / EDGE_B, corner_table(), all_pairs(): the operands.
  * Ref: the operations of the kernels under test on Python ints with `%` -- independent of lf_field.cuh and of the oracle's fast reduction.
  * classes_fp() / classes_fp3(): which branches a product takes, as predicates on the operands that mirror the structure of the code without calling it
    (tests/test_field_corners_cpu.py proves with them that every GPU case reaches every corner).

The case builders at the end are shared by tests/test_field_corners_cpu.py (reference against oracle, coverage) and tests/test_gpu_field_corners.py (device
against reference), so both see the same tables."""
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
FP_CLASSES = ("borrow", "hl0", "carry", "loose")
FP3_CLASSES = ("s128_up", "s128_down", "s128_loose")
CLASSES = FP_CLASSES + FP3_CLASSES


def grid(ring="goldilocks"):
    return EDGE_G if ring == "goldilocks" else EDGE_B


def corner_table(seed, shape, ring="goldilocks"):
    """canonical residues of the given shape: three extension-field elements in five (element e = word index // tau, chosen when (7 e + e // 8) % 5 < 3) have ALL
    their words on the grid, each picked by a SplitMix64 word -- the wraps of fq_from_s128 need whole grid operands --; the other elements are splitmix_fq words"""
    n = int(np.prod(shape))
    g = np.array(grid(ring), dtype=np.uint64)
    w = splitmix_fq(seed, 0, n, ring)
    pick = splitmix_fq(seed ^ 0xC0121E25, n, n, "goldilocks")
    e = np.arange(n, dtype=np.uint64) // np.uint64(RINGS[ring][2])
    edge = ((np.uint64(7) * e + e // np.uint64(8)) % np.uint64(5)) < np.uint64(3)
    return np.where(edge, g[(pick >> np.uint64(17)) % np.uint64(len(g))], w).reshape(shape)


def grid_share(a, ring="goldilocks"):
    return float(np.isin(np.asarray(a, dtype=np.uint64), np.array(grid(ring), dtype=np.uint64)).mean())


def all_pairs(ring="goldilocks"):
    """(A, B): ring elements whose slot-wise products enumerate grid x grid in every pair of coordinate positions (rotation 0: a = (x, .., x), b = (y, .., y); the
    other tau - 1 rotations mix the grid over the coordinates).  The last element is padded with the first pairs."""
    _p, RE, tau = RINGS[ring]
    g = grid(ring)
    ng = len(g)
    a, b = [], []
    for sh in range(tau):
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
    distinct (prefix, factor) pairs are those of the doubling recursion); from 6 on two half tables are built that way and multiplied entry by entry (k_eq_outer)"""
    nv = len(pt)
    if nv < 6:
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
    T = [elems(t[:2 * npairs]) for t in tabs]
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


def point(kind, nv, ring="goldilocks", shift=0):
    """nv extension-field coordinates: "grid" walks the grid, "pm1" / "half" are all p - 1 / all (p + 1) / 2, "bits" a 0 / 1 point"""
    p, _RE, tau = RINGS[ring]
    g = grid(ring)
    if kind == "grid":
        return np.array([[g[(shift + 5 * j + 3 * q) % len(g)] for q in range(tau)] for j in range(nv)], dtype=np.uint64)
    if kind == "pm1":
        return np.full((nv, tau), p - 1, dtype=np.uint64)
    if kind == "half":
        return np.full((nv, tau), (p + 1) // 2, dtype=np.uint64)
    assert kind == "bits"
    pt = np.zeros((nv, tau), dtype=np.uint64)
    pt[:, 0] = (np.arange(nv) + shift) % 2
    return pt


def challenges(n, ring="goldilocks"):
    """n round challenges from the grid; the first three put 0, 1 and p - 1 into every coordinate"""
    p, _RE, tau = RINGS[ring]
    g = grid(ring)
    sp = [0, 1, p - 1]
    out = [[sp[(k + q) % 3] for q in range(tau)] for k in range(3)]
    out += [[g[(7 * k + 4 * q + 1) % len(g)] for q in range(tau)] for k in range(3, n)]
    return np.array(out[:n], dtype=np.uint64)


def table(kind, seed, shape, ring="goldilocks"):
    return corner_table(seed, shape, ring) if kind == "corner" else np.full(shape, RINGS[ring][0] - 1, dtype=np.uint64)


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
