"""Python-integer references of the gadget maps on arrays (include/lfplus.h: lfplus_balanced_decompose, lfplus_balanced_recompose, lfplus_linf_norm,
lfplus_set_matrices_gadget), shared by tests/test_lfplus_digits_cpu.py and tests/test_gpu_lfplus_digits.py.  The digit rule is restated here with the
truncating division written out on Python integers (no int64 anywhere): centre to (-p/2, p/2), then k times q = trunc(cur / b), rem = cur - q b, and a
remainder with |rem| > floor(b / 2) moves one b towards zero (rem -+ b, q +- 1).  |rem| == b / 2 is kept, so a tie keeps the sign of the value."""
import numpy as np

P = 15912092521325583641
D = 16
GADGET, PLANES = 0, 1
BASES = (2, 3, 4, 10, 14, 2**31, 10**9 + 7, 2**62)
DIGITS = (1, 2, 16, 64)


def centre(v):
    v = int(v)
    return v if v <= (P - 1) // 2 else v - P


def tdivmod(a, b):
    """truncating division: the quotient rounds towards zero, the remainder has the sign of a"""
    q = abs(a) // b
    q = -q if a < 0 else q
    return q, a - q * b


def digits(v, b, k):
    """the k balanced base-b digits (signed integers, least significant first) of the field word v, and what is left of the value after them"""
    cur, half, out = centre(v), b // 2, []
    for _ in range(k):
        q, rem = tdivmod(cur, b)
        if abs(rem) > half:
            if rem < 0:
                rem, q = rem + b, q - 1
            else:
                rem, q = rem - b, q + 1
        out.append(rem)
        cur = q
    return out, cur


def corner_values(b, k):
    """0, +-1, +-floor(b/2), +-(floor(b/2) + 1), +-(b^k - 1)/2 where it is a centred field value, (p - 1)/2, (p + 1)/2 and p - 1, as canonical words"""
    half = b // 2
    vals = [0, 1, -1, half, -half, half + 1, -(half + 1)]
    top = (b**k - 1) // 2
    if top <= (P - 1) // 2:
        vals += [top, -top]
    return [v % P for v in vals] + [(P - 1) // 2, (P + 1) // 2, P - 1]


def rand_words(seed, count):
    """seeded canonical words (splitmix64 reduced mod p)"""
    out, x = [], seed & (2**64 - 1)
    for _ in range(count):
        x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        out.append((z ^ (z >> 31)) % P)
    return out


def operands(seed, count, b, k, pool=1024):
    """(count, 16) words: the corner grid (rotated by the seed, so that a single element sees another part of it) among seeded random words drawn from a pool
    of `pool` distinct ones -- the reference then costs one digit run per distinct word"""
    corners = corner_values(b, k)
    rnd = rand_words(seed, pool)
    pick = rand_words(seed ^ 0x5151, count * D)
    words = [corners[(i + seed) % len(corners)] if i < len(corners) or pick[i] % 5 == 0 else rnd[pick[i] % pool] for i in range(count * D)]
    return np.array(words, dtype=np.uint64).reshape(count, D)


def _place(dig, count, k, layout):
    """dig (count, k, 16) -> (count k, 16) in the layout"""
    return np.ascontiguousarray(dig.reshape(count * k, D) if layout == GADGET else dig.transpose(1, 0, 2).reshape(count * k, D))


def decompose(x, b, k, layout):
    """lfplus_balanced_decompose on a (count, 16) array -> (count k, 16) canonical residues of the digits (one digit run per distinct word)"""
    x = np.asarray(x, dtype=np.uint64).reshape(-1, D)
    u, inv = np.unique(x, return_inverse=True)
    table = np.array([[d % P for d in digits(int(v), b, k)[0]] for v in u], dtype=np.uint64)      # (distinct, k)
    dig = table[inv.reshape(-1)].reshape(x.shape[0], D, k)
    return _place(np.ascontiguousarray(dig.transpose(0, 2, 1)), x.shape[0], k, layout)


def kept(x, b, k):
    """the value the k digits carry: v minus b^k times what is left (v itself when it fits), word by word mod p"""
    x = np.asarray(x, dtype=np.uint64).reshape(-1, D)
    u, inv = np.unique(x, return_inverse=True)
    table = np.array([(centre(int(v)) - digits(int(v), b, k)[1] * b**k) % P for v in u], dtype=np.uint64)
    return table[inv.reshape(-1)].reshape(x.shape)


def recompose(x, b, k, layout):
    """lfplus_balanced_recompose on (count k, 16) GENERAL words -> (count, 16): sum_i b^i x[digit i], mod p"""
    x = np.asarray(x, dtype=np.uint64).reshape(-1, D)
    count = x.shape[0] // k
    planes = x.reshape(count, k, D).transpose(1, 0, 2) if layout == GADGET else x.reshape(k, count, D)
    acc = np.zeros((count, D), dtype=object)
    for i in range(k):
        acc = acc + planes[i].astype(object) * pow(b, i, P)
    return (acc % P).astype(np.uint64)


def linf(x):
    return max(abs(centre(int(v))) for v in np.asarray(x, dtype=np.uint64).reshape(-1))


def gadget_csr(mat, b, k, n):
    """the gadget form of a short CSR matrix (rows x m), padded to n rows: coefficient c at (r, j) -> c b^i mod p at (r, j k + i), entry e -> entries e k + i"""
    rowptr, col, val = (np.asarray(a) for a in mat)
    rows = rowptr.size - 1
    ncol, nval = [], []
    for e in range(col.size):
        for i in range(k):
            ncol.append(int(col[e]) * k + i)
            nval.append([int(c) * pow(b, i, P) % P for c in val[e]])
    nrp = [int(rowptr[min(r, rows)]) * k for r in range(n + 1)]
    return (np.array(nrp, dtype=np.uint32), np.array(ncol, dtype=np.uint32).reshape(-1), np.array(nval, dtype=np.uint64).reshape(-1, D))
