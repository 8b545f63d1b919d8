"""Corner operands, a Python-integer reference and a branch model for F_p of the Frog ring on the device (latticefold_amd/csrc/lfp_field.cuh).
TEST INFRASTRUCTURE ONLY (imported by name, like field_corners.py).

The LatticeFold+ kernels multiply Montgomery words (R = 2^64, p = 15912092521325583641 > 2^63): mont_mul, add_p, sub_p and the lazy 160-bit sums Acc160.  Random
canonical operands reach three of the classes (cy, o1, o2, v >= p) of mont_mul; cy = 0 needs a b = 0 (mod 2^64), o2 = 1 needs a b + m p = 2^128 exactly.  The
operands below reach them.  Four things live here:

  * GRID, PAIRS, ADD_CORNERS, SUB_CORNERS, W1_SUB2, canon_of_word(), mono(): the operands.  GRID is a grid of DEVICE WORDS; canon_of_word(w) = w 2^-64 mod p is the
    canonical value whose Montgomery form is w, so an entry point that converts an operand with to_mont sees exactly w.
  * the reference: Python integers and `%` (rmul / comb / prove_round / fix of lfplus_mlsumcheck_ref, and scalar_mul, tensor, tensor_product, spmv, decompose2
    here).  It knows nothing of Montgomery form.
  * the branch model: Dev -- the device's mont_mul / add_p / sub_p / Acc160 restated on Python integers, recording which branch every call takes under the name
    of the running case -- and dev_*(): the kernels' use of these functions, call by call.  It proves REACHABILITY (tests/test_lfp_field_corners_cpu.py) and is
    never the source of an expected value.
  * the cases shared by tests/test_lfp_field_corners_cpu.py (reference against the oracle, coverage) and tests/test_gpu_lfp_field_corners.py (device against
    the reference), so both see the same tables."""
import random

import numpy as np

import lfplus_mlsumcheck_ref as ref

P, D = 15912092521325583641, 16
M32, M64, M128 = 1 << 32, 1 << 64, 1 << 128
R = M64 % P                        # Montgomery 1 = 2^64 - p
R2 = pow(2, 128, P)
RINV = pow(M64, -1, P)
PINV = (-pow(P, -1, M64)) % M64
assert R == M64 - P and P * ((-PINV) % M64) % M64 == 1


def canon_of_word(w):
    """device word -> the canonical value whose Montgomery form it is: w 2^-64 mod p"""
    return w * RINV % P


def word_of(x):
    """canonical value -> its Montgomery word"""
    return x * M64 % P


def _dedupe(xs):
    return list(dict.fromkeys(xs))


_LIMB_HI = 0xFFFFFFFF00000000 if 0xFFFFFFFF00000000 < P else (P >> 32) << 32      # the largest word below p whose low limb is zero
GRID = _dedupe([0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, M32 - 1, M32, M32 + 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, R, R - 1, R + 1, R2, P - R2,
                0x5555555555555555, 0x00000000FFFFFFFF, _LIMB_HI] + ([(M64 // 3) * 2] if (M64 // 3) * 2 < P else []))
assert all(0 <= w < P for w in GRID) and 3 * 0x5555555555555555 == M64 - 1
NG = len(GRID)


# ---- the branch model -----------------------------------------------------------------------------------------------------------------------------------------
VFULL_BOUNDS = {P - 1: "p-1", P + 1: "p+1", M64 - 1: "2^64-1", M64: "2^64", M64 + 1: "2^64+1"}
MONT_COMMON = ((1, 0, 0, 0), (1, 0, 0, 1), (1, 1, 0, 0))


def mont_model(a, b):
    """((cy, o1, o2, v >= p), v_full, result) of mont_mul(a, b) as lfp_field.cuh forms it"""
    assert 0 <= a < P and 0 <= b < P
    pr = a * b
    lo, hi = pr % M64, pr >> 64
    m = lo * PINV % M64
    mh, ml = (m * P) >> 64, (m * P) % M64
    cy = int(lo + ml >= M64)
    assert (lo + ml) % M64 == 0
    u = hi + mh
    o1, u = int(u >= M64), u % M64
    v = u + cy
    o2, v = int(v >= M64), v % M64
    vfull = (pr + m * P) >> 64
    ge = int(v >= P)
    if o1 or o2 or ge:
        v = (v - P) % M64
    assert vfull == v + P * (o1 | o2 | ge) and v == pr * RINV % P
    return (cy, o1, o2, ge), vfull, v


def zero_low_limbs(pr):
    """how many of the four 32-bit limbs of a 128-bit product are zero from the bottom (4: the zero product)"""
    k = 0
    while k < 4 and (pr >> (32 * k)) % M32 == 0:
        k += 1
    return k


class Dev:
    """mont_mul, add_p, sub_p and Acc160 of lfp_field.cuh on Python integers.  hits[label] is the set of case names that reached the label:
      mont (cy, o1, o2, ge) / "mont cy0 nonzero" / "vfull <bound>";  "add none|ge|wrap", "add =p|=p-1|=2^64-1|=2^64";  "sub ge|lt", "sub a=b|0-(p-1)|a=b-1";
      signed sums "s neg zl<k>", "s pos zl", "s borrow5", "s carry5", "s w<w0>=p><w1>=p>", "s w4 below|notbelow";  unsigned sums "u carry5", "u w..", "u mult p"."""

    def __init__(self):
        self.hits = {}
        self.case = None

    def hit(self, label):
        self.hits.setdefault(label, set()).add(self.case)

    def supplied(self, label, case=None):
        s = self.hits.get(label, set())
        return bool(s) if case is None else case in s

    def mont_mul(self, a, b):
        cls, vfull, v = mont_model(a, b)
        self.hit(("mont",) + cls)
        if cls[0] == 0 and a * b:
            self.hit("mont cy0 nonzero")
        if vfull in VFULL_BOUNDS:
            self.hit("vfull " + VFULL_BOUNDS[vfull])
        return v

    def to_mont(self, a):
        return self.mont_mul(a, R2)

    def mul_p(self, a, b):
        return self.mont_mul(self.mont_mul(a, b), R2)

    def add_p(self, a, b):
        s = a + b
        self.hit("add wrap" if s >= M64 else "add ge" if s >= P else "add none")
        for v, name in ((P, "=p"), (P - 1, "=p-1"), (M64 - 1, "=2^64-1"), (M64, "=2^64")):
            if s == v:
                self.hit("add " + name)
        return s - P if s >= P else s

    def sub_p(self, a, b):
        self.hit("sub ge" if a >= b else "sub lt")
        if a == b:
            self.hit("sub a=b")
        if a == 0 and b == P - 1:
            self.hit("sub 0-(p-1)")
        if a == b - 1:
            self.hit("sub a=b-1")
        return (a - b) % P

    def acc(self, bias=0):
        return _Acc(self, bias)


BIAS16, BIAS1024 = 16 * P * M64, 1024 * P * M64


class _Acc:
    """the running 160-bit integer of a lazy sum, from its bias"""

    def __init__(self, dev, bias):
        self.dev, self.v, self.bias, self.k = dev, bias, bias, "s" if bias else "u"

    def mad(self, x, y, neg=False):
        pr, d, low = x * y, self.dev, self.v % M128
        if neg:
            d.hit(f"s neg zl{zero_low_limbs(pr)}")
            if low < pr:
                d.hit("s borrow5")
            self.v -= pr
        else:
            if pr and pr % M32 == 0:
                d.hit(self.k + " pos zl")
            if low + pr >= M128:
                d.hit(self.k + " carry5")
            self.v += pr
        assert 0 <= self.v < 1 << 160

    def red(self):
        d, v = self.dev, self.v
        w0, w1, w4 = v % M64, (v >> 64) % M64, v >> 128
        d.hit(f"{self.k} w{int(w0 >= P)}{int(w1 >= P)}")
        if self.bias:
            d.hit("s w4 below" if w4 < self.bias >> 128 else "s w4 notbelow")
        elif v and v % P == 0:
            d.hit("u mult p")
        for name, x0, x1 in (("w0", w0, w1 - P * (w1 >= P)), ("w1", w0 - P * (w0 >= P), w1)):      # would the result differ without this word's reduction?
            if _add_raw(_add_raw(_mont_raw(x0, 1), x1), _mont_raw(w4, R2)) != v * RINV % P:
                d.hit(f"{self.k} {name} reduction needed")
        w0, w1 = w0 - P * (w0 >= P), w1 - P * (w1 >= P)
        out = d.add_p(d.add_p(d.mont_mul(w0, 1), w1), d.mont_mul(w4, R2))
        assert out == v * RINV % P
        return out


def _add_raw(a, b):
    """add_p on any 64-bit words, as the device computes it"""
    s = (a + b) % M64
    return (s - P) % M64 if s < a or s >= P else s


def _mont_raw(a, b):
    """mont_mul on any 64-bit words, as the device computes it"""
    pr = a * b
    lo, hi = pr % M64, pr >> 64
    m = lo * PINV % M64
    cy = int(lo + (m * P) % M64 >= M64)
    u = hi + ((m * P) >> 64)
    o1, u = u >= M64, u % M64
    v = u + cy
    o2, v = v >= M64, v % M64
    return (v - P) % M64 if o1 or o2 or v >= P else v


# ---- constructed pairs ----------------------------------------------------------------------------------------------------------------------------------------
def _pair_for_vfull(V, rng):
    """a, b < p with (a b + m p) / 2^64 = V: for a candidate a, m is determined mod a (m p = V 2^64 mod a) and is the one member of that class in the window
    that keeps b = (V 2^64 - m p) / a in [0, p); accepted when that m is below 2^64"""
    while True:
        a = rng.randrange(1 << 62, P)
        m0 = V * M64 * pow(P, -1, a) % a
        top = min(M64 - 1, V * M64 // P)
        m = top - (top - m0) % a
        if m < 0:
            continue
        b, rem = divmod(V * M64 - m * P, a)
        if rem == 0 and 0 < b < P and mont_model(a, b)[1] == V:
            return a, b


def _build_pairs():
    rng = random.Random(0x1F9C0)
    pairs = {"vfull " + name: _pair_for_vfull(V, rng) for V, name in VFULL_BOUNDS.items()}
    pairs["o2 issue"] = (14880340936552667056, 7603427346964385809)
    pairs.update({"cy0 2^32 2^32": (M32, M32), "cy0 2^63 2": (1 << 63, 2), "cy0 2^33 3*2^31": (1 << 33, 3 << 31), "cy0 2^32 2^63": (M32, 1 << 63)})
    for V in (P - 1, P + 1):
        pairs["to_mont " + VFULL_BOUNDS[V]] = (V * M64 * pow(R2, -1, P) % P, R2)
    return pairs


PAIRS = _build_pairs()


def _w1_terms(bias, signs, rng, same_y=False):
    """words (W_i, y_i) whose products, entering a lazy sum from `bias` with the given signs, leave the middle word w1 in [p, 2^64) AND make its reduction
    matter: without `if (w1 >= P) w1 -= P` acc160_red would return another word.  (That needs w1 >= p, mont_mul(w0, 1) + w1 - p >= p and a fifth word whose
    image w4 2^64 mod p is large -- 12 from the bias of 16: single products and most pseudo-random sums do not get there.)"""
    while True:
        terms = [(rng.randrange(P // 2, P), rng.randrange(P // 2, P)) for _ in signs]
        if same_y:
            terms = [(w, terms[0][1]) for w, _ in terms]
        d = Dev()
        n = d.acc(bias)
        for (w, y), neg in zip(terms, signs):
            n.mad(w, y, neg)
        n.red()
        if d.supplied("s w1 reduction needed"):
            return terms


_rng = random.Random(0x31F)
W1_SUB2 = [_w1_terms(16 * P * M64, (True,) * 2, _rng, same_y=True) for _ in range(2)]      # one negacyclic product: (w1 X^15 + w2 X^14) times a row of y
                                                                                         # subtracts w1 y and w2 y in coefficients 0..13, from the bias of 16
for _n, (_a, _b) in PAIRS.items():
    _c, _v, _ = mont_model(_a, _b)
    assert (not _n.startswith("vfull") and not _n.startswith("to_mont")) or VFULL_BOUNDS[_v] == _n.split()[1], _n
    assert not _n.startswith("cy0") or (_c[0] == 0 and _a * _b), _n
    assert not _n.startswith("o2") or (_c == (1, 0, 1, 0) and _v == M64), _n
assert mont_model(*PAIRS["vfull 2^64"])[0] == (1, 0, 1, 0)
PAIR_A, PAIR_B = [a for a, _ in PAIRS.values()], [b for _, b in PAIRS.values()]
ADD_CORNERS = {"=p": ((P + 1) // 2, (P - 1) // 2), "=p-1": (P - 2, 1), "=2^64-1": (P - 1, M64 - P), "=2^64": (P - 1, M64 - P + 1)}
SUB_CORNERS = {"a=b": (R2, R2), "0-(p-1)": (0, P - 1), "a=b-1": (M32 - 1, M32)}
assert all(a < P and b < P and a > M64 - P for a, b in (ADD_CORNERS["=2^64"],))


# ---- the reference: Python integers --------------------------------------------------------------------------------------------------------------------------
def u64(a):
    return np.array(a, dtype=object).astype(np.uint64) if not isinstance(a, np.ndarray) or a.dtype == object else a


def scalar_mul(a, b):
    return int(a) * int(b) % P


def tensor_product(a, b):
    """utils::tensor_product: out[i n + j] = a_i b_j"""
    return u64([scalar_mul(x, y) for x in a for y in b])


def tensor(r):
    """utils::tensor: (1 - r_0, r_0) (x) (1 - r_1, r_1) (x) ..., the first coordinate outermost"""
    out = [1]
    for x in r:
        out = [v * w % P for v in out for w in ((1 - int(x)) % P, int(x) % P)]
    return u64(out)


def spmv(mat, x):
    """CSR x vector of ring elements"""
    rowptr, col, val = mat
    out = np.zeros((len(rowptr) - 1, D), dtype=object)
    for r in range(len(rowptr) - 1):
        for k in range(int(rowptr[r]), int(rowptr[r + 1])):
            out[r] = out[r] + ref.rmul(val[k], x[int(col[k])])
    return (out % P).astype(np.uint64)


def ring_mul_sum(a, b, broadcast):
    """sum_i a_i * b_i: a (T, count, 16); b (T, count, 16), or (T, 16) with broadcast"""
    acc = np.zeros(a.shape[1:], dtype=object)
    for i in range(a.shape[0]):
        acc = acc + ref.rmul(a[i], b[i][None, :] if broadcast else b[i])
    return (acc % P).astype(np.uint64)


def centre(w):
    w = int(w)
    return w - P if w > (P - 1) // 2 else w


def decompose2(f, B):
    """the two balanced base-B digits of every centred coefficient (decomp.rs:32-99, two digits): the quotient rounds towards zero, the remainder has the sign
    of the value and moves by B (the quotient by one) when it exceeds floor(B / 2) in magnitude -- an exact tie +-B/2 stays; -> (F0, F1) canonical"""
    F0, F1 = [], []
    for w in np.asarray(f).reshape(-1):
        cur, dig = centre(w), []
        for _ in range(2):
            sign, mag = (-1 if cur < 0 else 1), abs(cur)
            r = sign * (mag % B)
            cur = sign * (mag // B)
            if abs(r) > B // 2:
                r -= sign * B
                cur += sign
            dig.append(r)
        F0.append(dig[0] % P); F1.append(dig[1] % P)
    sh = np.asarray(f).shape
    return u64(F0).reshape(sh), u64(F1).reshape(sh)


def decompose_identities(f, F0, F1, B):
    """-> (holds, how many words fit): |F0| <= B / 2 for every word; for the words within two balanced digits (|f| <= floor(B / 2) (B + 1)): f = F0 + B F1 over
    the integers and |F1| <= B / 2"""
    h, ok, fits = B // 2, True, 0
    for w, d0, d1 in zip(np.asarray(f).reshape(-1), np.asarray(F0).reshape(-1), np.asarray(F1).reshape(-1)):
        c, c0, c1 = centre(w), centre(d0), centre(d1)
        ok = ok and abs(c0) <= h and (c - c0) % B == 0
        if abs(c) <= h * (B + 1):
            fits += 1
            ok = ok and c == c0 + B * c1 and abs(c1) <= h
    return ok, fits


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------------------------
def mono(alpha, j):
    """alpha X^j"""
    e = [0] * D
    e[j] = int(alpha) % P
    return e


def grid_row(shift, step=1):
    return [GRID[(shift + step * c) % NG] for c in range(D)]


def rows_u64(rows):
    """nested lists of Python integers -> uint64 words; every table of every case comes through here, so every word is canonical"""
    a = np.array(rows, dtype=object)
    assert ((a >= 0) & (a < P)).all(), "non-canonical word in a case table"
    return a.astype(np.uint64)


# ---- the kernels' use of the field functions, call by call (branch model only) -------------------------------------------------------------------------------
def dev_tensor_product(dev, a, b):
    """k_tensor_product: mul_p(a_i, b_j) = mont_mul(mont_mul(a_i, b_j), R2)"""
    return [dev.mul_p(int(x), int(y)) for x in a for y in b]


def dev_tensor(dev, r):
    """k_tensor_level per coordinate: mul_p(v, 1 - r), mul_p(v, r); 1 - r is formed without sub_p (r <= 1 ? 1 - r : p + 1 - r)"""
    cur = [1]
    for x in r:
        x = int(x) % P
        om = 1 - x if x <= 1 else P + 1 - x
        cur = [w for v in cur for w in (dev.mul_p(v, om), dev.mul_p(v, x))]
    return cur


def _negacyclic(dev, xM, y, bias):
    """one lazy signed sum per output coefficient: acc160_mad_signed(n, xM[j], y[(c - j) & 15], j > c) for j = 0..15, then acc160_red"""
    out = []
    for c in range(D):
        n = dev.acc(bias)
        for j in range(D):
            n.mad(xM[j], y[(c - j) & 15], j > c)
        out.append(n.red())
    return out


def dev_ring_mul(dev, a, b, broadcast):
    """k_ring_mul: mode 0 converts a on the device (to_mont); mode 1 takes b in Montgomery form from the host.  One sum over all terms from the bias 1024 p 2^64"""
    T, count = a.shape[0], a.shape[1]
    out = []
    for x in range(count):
        accs = [dev.acc(BIAS1024) for _ in range(D)]
        for i in range(T):
            if broadcast:
                xM, y = [word_of(int(w)) for w in b[i]], [int(w) for w in a[i, x]]
            else:
                xM, y = [dev.to_mont(int(w)) for w in a[i, x]], [int(w) for w in b[i, x]]
            for c in range(D):
                for j in range(D):
                    accs[c].mad(xM[j], y[(c - j) & 15], j > c)
        out.append([n.red() for n in accs])
    return out


def dev_spmv(dev, mat, x):
    """k_spmv_ring / k_spmv_ring_const on a matrix whose values went to Montgomery form on the device (launch_to_mont)"""
    rowptr, col, val = mat
    const = not np.asarray(val)[:, 1:].any()
    valM = [[dev.to_mont(int(w)) for w in v] for v in val]
    out = []
    for r in range(len(rowptr) - 1):
        acc = [0] * D
        for k in range(int(rowptr[r]), int(rowptr[r + 1])):
            xr = [int(w) for w in x[int(col[k])]]
            for t in range(D):
                if const:
                    acc[t] = dev.add_p(acc[t], dev.mont_mul(valM[k][0], xr[t]))
                else:
                    lane = 0
                    for s in range(D):
                        pr = dev.mont_mul(valM[k][s], xr[(t - s) & 15])
                        lane = dev.sub_p(lane, pr) if t - s < 0 else dev.add_p(lane, pr)      # (the subtraction is written out in ring_mul_lane: the branches of sub_p)
                    acc[t] = dev.add_p(acc[t], lane)
        out.append(acc)
    return out


def dev_mls(dev, tables, terms, degree, challenges):
    """k_mls_round (round 1 on the tables, later rounds fused with the fix at the previous challenge) and k_mls_final -> (messages, final values)"""
    cur = [[[int(w) for w in e] for e in t] for t in np.asarray(tables)]
    nvars = len(cur[0]).bit_length() - 1
    cf = [[int(w) for w in np.asarray(c).reshape(D)] if not isinstance(c, (int, np.integer)) else [int(c) % P] + [0] * 15 for c, _ in terms]
    cls = ["zero" if not any(c) else "one" if c[0] == 1 and not any(c[1:]) else "minus" if c[0] == P - 1 and not any(c[1:]) else "general" for c in cf]
    fixw = lambda rM, lo, hi: dev.add_p(lo, dev.mont_mul(rM, dev.sub_p(hi, lo)))
    msgs = []
    for rnd in range(nvars):
        if rnd:
            rM = word_of(int(challenges[rnd - 1]))
            cur = [[[fixw(rM, t[2 * j][c], t[2 * j + 1][c]) for c in range(D)] for j in range(len(t) // 2)] for t in cur]
        half = len(cur[0]) // 2
        tot = [[[0] * D for _ in range(degree + 1)] for _ in range(16)]
        for b in range(half):
            val = [[t[2 * b][c] for c in range(D)] for t in cur]
            st = [[dev.sub_p(t[2 * b + 1][c], t[2 * b][c]) for c in range(D)] for t in cur]
            for x in range(degree + 1):
                if x:
                    val = [[dev.add_p(v[c], s[c]) for c in range(D)] for v, s in zip(val, st)]
                sums = [0] * D
                for i, (_, idx) in enumerate(terms):
                    if cls[i] == "zero":
                        continue
                    v = val[idx[0]]
                    for k in idx[1:]:
                        v = _negacyclic(dev, [dev.to_mont(w) for w in v], val[k], BIAS16)
                    if cls[i] == "general":
                        v = _negacyclic(dev, [dev.to_mont(w) for w in v], cf[i], BIAS16)
                    sums = [dev.sub_p(s, w) if cls[i] == "minus" else dev.add_p(s, w) for s, w in zip(sums, v)]
                tot[b][x] = [dev.add_p(0, s) for s in sums]
        msg = []
        for x in range(degree + 1):
            row = []
            for c in range(D):
                t = 0
                for p in range(16):
                    t = dev.add_p(t, tot[p][x][c])
                row.append(t)
            msg.append(row)
        msgs.append(msg)
    rM = word_of(int(challenges[nvars - 1]))
    return msgs, [[fixw(rM, t[0][c], t[1][c]) for c in range(D)] for t in cur]


def dev_row_gather(dev, mat, valM, const, f, row):
    rowptr, col, _ = mat
    if const:
        accs = [dev.acc(0) for _ in range(D)]
        for k in range(int(rowptr[row]), int(rowptr[row + 1])):
            for t in range(D):
                accs[t].mad(valM[k][0], int(f[int(col[k])][t]))
        return [n.red() for n in accs]
    g = [0] * D
    for k in range(int(rowptr[row]), int(rowptr[row + 1])):
        pr = _negacyclic(dev, valM[k], [int(w) for w in f[int(col[k])]], BIAS16)
        g = [dev.add_p(a, b) for a, b in zip(g, pr)]
    return g


def dev_r1cs_residual(dev, mats, f):
    """k_r1cs_residual: the three gathers (constant-coefficient matrices: one unsigned lazy sum per row and lane), to_mont(g_A), one signed sum per coefficient
    -> the rows with a non-zero residual"""
    vM = [[[dev.to_mont(int(w)) for w in v] for v in m[2]] for m in mats]
    const = [not np.asarray(m[2])[:, 1:].any() for m in mats]
    bad = []
    for row in range(len(mats[0][0]) - 1):
        ga, gb, gc = (dev_row_gather(dev, mats[q], vM[q], const[q], f, row) for q in range(3))
        if _negacyclic(dev, [dev.to_mont(w) for w in ga], gb, BIAS16) != gc:
            bad.append(row)
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------
TENSOR_POINTS = {"len1 0": [0], "len1 1": [1], "len1 p-1": [P - 1], "len2 to_mont": [PAIRS["to_mont p-1"][0], PAIRS["to_mont p+1"][0]],
                 "len3": [GRID[3], GRID[8], GRID[13]], "len4": [GRID[(5 * i + 2) % NG] for i in range(4)], "len5": [GRID[(7 * i + 1) % NG] for i in range(5)],
                 "len6": [0, 1, P - 1, PAIRS["to_mont p-1"][0], GRID[10], GRID[18]]}


def placed(w):
    """the canonical value an entry point must be given so that its to_mont produces the device word w"""
    return canon_of_word(w)


def ring_mul_cases():
    """name -> (a (T, count, 16), b, broadcast).  The a rows of the monomial cases are placed(w) X^j: to_mont gives the Montgomery word w in position j and zeros
    elsewhere, so output coefficient c of a row is the single term +-w y[(c - j) & 15] (and fifteen zero products, subtracted for j > c).  The rows of b
    walk the grid."""
    cases = {}
    for j, count in ((0, 17), (15, 33)):
        a = rows_u64([mono(placed(GRID[x % NG]), j) for x in range(count)])
        b = rows_u64([grid_row(3 * x + x // NG, 1 + x % 3) for x in range(count)])
        cases[f"mono{j}/count{count}"] = (a[None], b[None], False)
    # the constructed pairs: w = the first word, every coefficient of b the second; X^0 adds the product, X^15 subtracts it in coefficients 0..14
    npair = len(PAIRS)
    for j in (0, 15):
        a = rows_u64([mono(placed(PAIR_A[x % npair]), j) for x in range(17)])
        b = rows_u64([[PAIR_B[x % npair]] * D for x in range(17)])
        cases[f"pairs X^{j}"] = (a[None], b[None], False)
    # the sign chain: subtracted products whose low one, two, three limbs are zero (and the zero products of every monomial row)
    chain = [(M32, 1), (M32, M32), (M32, 1 << 63), (1 << 63, 1 << 63), (1 << 63, 2), (M32, 3), (_LIMB_HI, M32), (_LIMB_HI, _LIMB_HI)]
    a = rows_u64([mono(placed(chain[x % len(chain)][0]), 15 if x < 17 else 0) for x in range(33)])
    b = rows_u64([[chain[x % len(chain)][1]] * D for x in range(33)])
    cases["sign chain"] = (a[None], b[None], False)
    # sums of two and three chosen terms, element-wise and broadcast
    for T, count in ((2, 33), (3, 17)):
        a = rows_u64([[mono(placed(GRID[(x + 5 * i) % NG]), (0, 15, 7)[i]) for x in range(count)] for i in range(T)])
        b = rows_u64([[grid_row(x + 11 * i, 2) for x in range(count)] for i in range(T)])
        cases[f"terms{T}/count{count}"] = (a, b, False)
        bb = rows_u64([mono(GRID[(4 + 9 * i) % NG], (15, 0, 3)[i]) for i in range(T)])       # (mode 1: b is converted on the host; a stays canonical)
        cases[f"terms{T}/count{count}/broadcast"] = (b, bb, True)
    bb = rows_u64([grid_row(6, 5)])
    cases["grid rows/broadcast"] = (rows_u64([grid_row(2 * x + 1, 3) for x in range(33)])[None], bb, True)
    return cases


def add_chain_rows():
    """(x rows, (rowptr, col)) for a constant-coefficient matrix of ones: lane t of a row adds the words of its columns in order from 0.  Rows with two
    non-zeros put every add_p corner into a lane; the rows with five pass sum = p and sum = 2^64 in the middle of the chain"""
    corners = list(ADD_CORNERS.values())
    xa = [corners[t % 4][0] for t in range(D)]
    xb = [corners[t % 4][1] for t in range(D)]
    # five terms: 1, (p - 1) / 2, (p - 1) / 2 (sum = p -> 0), then p - 1 and 2^64 - p + 1 (sum = 2^64 -> 2^64 - p)
    five = [[1] * D, [(P - 1) // 2] * D, [(P - 1) // 2] * D, [P - 1] * D, [M64 - P + 1] * D]
    return [xa, xb] + five


def spmv_case():
    """n = 64 -> (matrices, x).  Matrix 0 has ring coefficients (monomials of placed grid words and placed grid rows), matrix 1 constant coefficients (placed
    grid words: the device's valMc is the grid word), matrix 2 is the constant matrix of ones whose rows run the add_p chains of add_chain_rows(); rows have
    0, 1, 2 and 5 non-zeros"""
    n = 64
    x = [grid_row(5 * r + r // NG, 1 + r % 4) for r in range(n)]
    chain = add_chain_rows()
    x[40:40 + len(chain)] = chain
    x[50] = [PAIR_B[t % len(PAIRS)] for t in range(D)]
    nnz = [(1, 2, 0, 5)[r % 4] for r in range(n)]
    rowptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.uint32)
    col = np.array([(7 * k + 3 * (k // 5)) % n for k in range(int(rowptr[-1]))], dtype=np.uint32)
    ring = rows_u64([mono(placed(GRID[k % NG]), (0, 15, 5)[k % 3]) if k % 4 else [placed(w) for w in grid_row(k, 3)] for k in range(col.size)])
    const = np.zeros((col.size, D), dtype=np.uint64)
    const[:, 0] = rows_u64([placed(GRID[(k * 5 + 1) % NG]) for k in range(col.size)])
    # the pairs: a row with one non-zero placed(first word) on column 50, whose lane t holds the second word of pair t
    pk = [int(rowptr[r]) for r in range(n) if nnz[r] == 1]
    assert len(pk) >= len(PAIRS)
    for t, k in enumerate(pk[:D]):
        const[k, 0], col[k] = placed(PAIR_A[t % len(PAIRS)]), 50
    ones_nnz = [(2, 5, 1, 0)[r % 4] for r in range(n)]
    orp = np.concatenate([[0], np.cumsum(ones_nnz)]).astype(np.uint32)
    ocol = []
    for r in range(n):
        ocol += {2: [40, 41], 5: [42, 43, 44, 45, 46], 1: [r], 0: []}[ones_nnz[r]]
    ones = np.zeros((len(ocol), D), dtype=np.uint64)
    ones[:, 0] = 1
    return [(rowptr, col, ring), (rowptr, col.copy(), const), (orp, np.array(ocol, dtype=np.uint32), ones)], rows_u64(x)


MLS_NVARS = (1, 4, 5)


def mls_case(nvars):
    """(tables (3, 2^nvars, 16), terms, degree, challenges): table 0 monomial rows of placed grid words (a term's first factor goes through to_mont), table 1
    grid rows, table 2 grid rows with the sub_p corners in its first pairs; coefficients from the grid (one general ring element, one general constant, 1 and
    p - 1); challenges from the grid: 0, 1, p - 1, the value whose Montgomery form is 2^32, the to_mont corner operands"""
    n = 1 << nvars
    t0 = [mono(placed(GRID[(3 * x + 1) % NG]), (0, 15, 0, 9)[x % 4]) for x in range(n)]
    t1 = [grid_row(2 * x + 7, 1 + x % 2) for x in range(n)]
    t2 = [grid_row(11 * x, 3) for x in range(n)]
    (w1, y), (w2, _) = W1_SUB2[0]                        # coefficients 0..13 of t0[0] t1[0] subtract w1 y and w2 y: the reduction of the middle word matters
    t0[0], t1[0] = [0] * 14 + [placed(w2), placed(w1)], [y] * D
    sc = list(SUB_CORNERS.values())
    t2[0] = [sc[c % 3][1] for c in range(D)]          # sub_p(v1, v0): v0 is the subtrahend
    t2[1] = [sc[c % 3][0] for c in range(D)]
    if n >= 4:
        t2[2], t2[3] = [M32] * D, [(2 * M32) % P] * D      # step 2^32 against the challenge whose Montgomery word is 2^32: cy = 0 in the fix
    coef = rows_u64([grid_row(4, 5), mono(GRID[12], 0)])
    terms = [(coef[0], [0, 1, 2]), (coef[1], [0, 0]), (1, [0, 1]), (P - 1, [2])]
    ch = [placed(M32), 0, 1, P - 1, PAIRS["to_mont p-1"][0], PAIRS["to_mont p+1"][0]]
    return rows_u64([t0, t1, t2]), terms, 3, ch[:nvars]


def r1cs_case():
    """n = 64: (matrices, witness f, the rows that carry each constructed pair).  Rows 0..31 are active: M_A gathers from f[0..16), M_B from f[16..32), M_C is
    identity-like and picks f[32 + row], where the reference's product g_A g_B is planted; rows 32..63 are empty in all three.  M_A has ring coefficients
    (monomials of placed words: one signed sum per non-zero), M_B constant coefficients (placed words: ONE unsigned lazy sum per row and lane over 1, 2 or 5
    non-zeros).  Row r < len(PAIRS): g_A = placed(first word of pair r), lane t of g_B = the second word of pair t, so coefficient r of the product row holds
    the pair's product as a term of its signed sum"""
    n = 64
    npair = len(PAIRS)
    f = [[0] * D for _ in range(n)]
    for r in range(16):
        f[r] = grid_row(3 * r + 1, 1 + r % 3)
        f[16 + r] = grid_row(5 * r + 2, 2)
    f[0] = [1] + [0] * 15                                   # the constant 1: M_A row r = placed(first word) X^0 times 1 -> g_A = placed(first word)
    f[16] = [PAIR_B[t % npair] for t in range(D)]           # M_B row r = 1 times f[16] -> lane t of g_B is the second word of pair t
    f[17] = [(P - w) % P for w in f[18]]               # f[17] + f[18] = p in every lane: an unsigned sum that is an exact multiple of p
    f[19], f[20] = [P - 1] * D, [1 << 63] * D               # (p - 1)(p - 1) + 2^63 2^63: both low words of the unsigned sum land in [p, 2^64)
    a_nnz = [1] * 32 + [0] * 32
    arp = np.concatenate([[0], np.cumsum(a_nnz)]).astype(np.uint32)
    acol = np.array([0 if r < npair else r % 16 for r in range(32)], dtype=np.uint32)
    aval = [mono(placed(PAIR_A[r]), 0) if r < npair else mono(placed(GRID[r % NG]), (15, 0, 4)[r % 3]) for r in range(32)]
    (w1, y), (w2, _) = W1_SUB2[1]                           # row 16: g_A = w1 X^15 + w2 X^14 (placed), g_B = a row of y: the middle-word reduction of the residual's sum matters
    acol[16], aval[16], f[21] = 0, [0] * 14 + [placed(w2), placed(w1)], [y] * D
    aval = rows_u64(aval)
    b_nnz = [1 if r < npair else (2, 5, 1)[r % 3] for r in range(32)] + [0] * 32
    brp = np.concatenate([[0], np.cumsum(b_nnz)]).astype(np.uint32)
    bcol, bval = [], []
    for r in range(32):
        if r < npair:
            bcol.append(16); bval.append(placed(R))        # the coefficient 1 (device word R): g_B = f[16] through an unsigned sum of R f
        elif b_nnz[r] == 2 and r % 2 == 0:
            bcol += [17, 18]; bval += [placed(1), placed(1)]      # device word 1: the sum is f[17] + f[18] = p exactly
        elif r == 15:
            bcol += [19, 20]; bval += [placed(P - 1), placed(1 << 63)]
        elif r == 16:
            bcol += [21] + [18] * 4; bval += [placed(R)] + [0] * 4       # (five non-zeros as the row pattern has it: the coefficient 1 and four zeros)
        else:
            for q in range(b_nnz[r]):
                bcol.append(16 + (r + 3 * q) % 16); bval.append(placed(GRID[(r + 7 * q) % NG] or P - 1) if q % 2 else P - 1 - q)
    bv = np.zeros((len(bcol), D), dtype=np.uint64)
    bv[:, 0] = rows_u64(bval)
    crp = np.concatenate([[0], np.cumsum(a_nnz)]).astype(np.uint32)
    ccol = np.arange(32, 64, dtype=np.uint32)
    cval = np.zeros((32, D), dtype=np.uint64)
    cval[:, 0] = 1
    mats = [(arp, acol, aval), (brp, np.array(bcol, dtype=np.uint32), bv), (crp, ccol, cval)]
    f = rows_u64(f)
    ga, gb = spmv(mats[0], f), spmv(mats[1], f)
    f[32:] = ref.rmul(ga, gb)[:32].astype(np.uint64)
    return mats, f, {name: r for r, name in enumerate(PAIRS)}


DECOMP_BASES = (7, 8, 50, 3989010971)


def decompose_f(B, n=1 << 10):
    """(n, 16) canonical words: centred-small values with the corner values of base B planted among them: (p - 1) / 2, (p + 1) / 2, +-floor(B / 2),
    +-(floor(B / 2) + 1), +-(B floor(B / 2) + floor(B / 2)) and their neighbours"""
    h = B // 2
    v = [((i * 2654435761) % (2 * h * h + 1)) - h * h if B < 1 << 20 else ((i * 0x9E3779B97F4A7C15) % (1 << 40)) - (1 << 39) for i in range(n * D)]
    corners = []
    for c in (h, h + 1, B * h + h, B, B * h, 1, 0):
        for d in (-1, 0, 1):
            corners += [c + d, -(c + d)]
    corners = [c for c in corners if abs(c) <= (P - 1) // 2] + [(P - 1) // 2, -((P - 1) // 2), (P - 1) // 2 - 1, -((P - 1) // 2 - 1)]
    for i, c in enumerate(corners):
        v[37 * i + 5] = c
    return rows_u64([x % P for x in v]).reshape(n, D), corners


CCS_CONST = placed(M32)              # a constant coefficient whose Montgomery word is 2^32
SHAPES = {"r1cs": (3, [[0, 1], [2]], [1, -1]), "deg3": (3, [[0, 1, 1], [2]], [CCS_CONST, -1])}


def shape_product(name, ga, gb):
    """the product row a satisfied instance of SHAPES[name] needs in g_C: g_A g_B, or c g_A g_B g_B"""
    pr = ref.rmul(ga, gb)
    if name == "deg3":
        pr = ref.rmul(pr, gb) * CCS_CONST % P
    return pr.astype(np.uint64)


def check_case(name):
    """the instance of r1cs_case() satisfied for SHAPES[name] -> (matrices, f, rows of the pairs)"""
    mats, f, rows = r1cs_case()
    f = f.copy()
    f[32:] = shape_product(name, spmv(mats[0], f), spmv(mats[1], f))[:32]
    return mats, f, rows


CHECK_BAD = ((0, 0, 1), (3, 3, -1), (5, 5, 1), (6, 6, -1), (15, 9, 1), (31, 15, -1))      # (row, word, change) of the rejected instances


def lin_case(name, nvars):
    """a satisfied instance of SHAPES[name] on n = 2^nvars rows with a witness from the grid: rows 0..n/2 are active, M_A (monomials of placed grid words) gathers
    from the first quarter of f, M_B (constant placed grid words, one or two per row) from the second, M_C picks f[n/2 + row] where the product is planted"""
    n = 1 << nvars
    q = n // 4
    f = [grid_row(3 * r + 1, 1 + r % 3) if r < 2 * q else [0] * D for r in range(n)]
    f[0] = [1] + [0] * 15
    f[q] = [PAIR_B[t % len(PAIRS)] for t in range(D)]
    act = [1] * (2 * q) + [0] * (2 * q)
    arp = np.concatenate([[0], np.cumsum(act)]).astype(np.uint32)
    acol = np.array([0 if r < 3 else r % q for r in range(2 * q)], dtype=np.uint32)
    aval = rows_u64([mono(placed(PAIR_A[(3, 5, 6)[r]]), 0) if r < 3 else mono(placed(GRID[(2 * r + 1) % NG]), (15, 0, 4)[r % 3]) for r in range(2 * q)])
    b_nnz = [1 if r < 3 else 1 + r % 2 for r in range(2 * q)] + [0] * (2 * q)
    brp = np.concatenate([[0], np.cumsum(b_nnz)]).astype(np.uint32)
    bcol, bval = [], []
    for r in range(2 * q):
        for k in range(b_nnz[r]):
            bcol.append(q if r < 3 else q + (r + k) % q)
            bval.append(placed(R) if r < 3 else placed(GRID[(r + 5 * k + 3) % NG]))
    bv = np.zeros((len(bcol), D), dtype=np.uint64)
    bv[:, 0] = rows_u64(bval)
    cval = np.zeros((2 * q, D), dtype=np.uint64)
    cval[:, 0] = 1
    mats = [(arp, acol, aval), (brp, np.array(bcol, dtype=np.uint32), bv), (arp.copy(), np.arange(2 * q, n, dtype=np.uint32), cval)]
    f = rows_u64(f)
    f[2 * q:] = shape_product(name, spmv(mats[0], f), spmv(mats[1], f))[:2 * q]
    return mats, f


def mle_const(f, r):
    """mle(f)(r) for a point of constants (Python integers), bit 0 of the row index <-> r[0]"""
    tab = np.asarray(f).astype(object)
    for x in r:
        tab = (tab[0::2] + int(x) * (tab[1::2] - tab[0::2])) % P
    return tab[0].astype(np.uint64)


def linb_case():
    """nvars = 10 -> (f, r (10, 2, 16), matrices, v (2, 2, 16)): every word of f from the grid, both points constants whose Montgomery words are grid words (0, 1
    and p - 1 among them), one constant-coefficient diagonal matrix of placed grid words; v = the reference's evaluations of f and M f"""
    nvars, n = 10, 1 << 10
    f = rows_u64([grid_row(r + 2 * (r // NG), 1 + r % 5) for r in range(n)])
    r = np.zeros((nvars, 2, D), dtype=np.uint64)
    words = [[0, R, P - R, M32, GRID[5], GRID[10], GRID[13], GRID[16], GRID[18], GRID[19]], [GRID[(3 * j + 4) % NG] for j in range(nvars)]]
    for pt in range(2):
        r[:, pt, 0] = rows_u64([placed(w) for w in words[pt]])
    val = np.zeros((n, D), dtype=np.uint64)
    val[:, 0] = rows_u64([placed(GRID[(7 * i + 2) % NG]) for i in range(n)])
    mat = (np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), val)
    Mf = (f.astype(object) * val[:, :1].astype(object) % P).astype(np.uint64)
    v = np.stack([np.stack([mle_const(t, r[:, pt, 0]) for pt in range(2)]) for t in (f, Mf)])
    return f, r, [mat], v


def range_check_matrix(n):
    """identity-like, constant coefficients: the diagonal cycles through placed grid words (none of them zero)"""
    g = [w for w in GRID if w]
    val = np.zeros((n, D), dtype=np.uint64)
    val[:, 0] = rows_u64([placed(g[i % len(g)]) for i in range(n)])
    return np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), val

