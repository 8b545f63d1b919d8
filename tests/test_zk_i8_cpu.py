"""The byte-cut matrix of the z_k build (csrc/lf_zk_i8.hip) on integers, without a GPU: the CRT of the oracle's tables times B^l for one residue class of the
coefficient index, every entry cut into eight balanced base-256 digits, restated in numpy in the kernel's operand and register order -- A bytes
[class][tile][lane][16], B bytes = the digits (q, l) of one element per lane, C register 4 j + r of lane (n, h) = row 8 j + 4 h + r = (p, byte) = (2 j + h,
r + 4 tile) -- with the biased recombination X + 2^24 (Y + 2^24 Z) = word + 17 p, against lfo.crt(lfo.recompose(...)) of the same digit planes."""
import numpy as np
import pytest

import lfo

P = lfo.P
K = 16
NEL = 32                                     # one tile: the 32 columns of a wave
REACH = 0x7F7F7F7F7F7F7F7F                   # the largest integer eight balanced digits express


def _matrix(B):
    """what zk_i8_prepare derives: the answers U [96][24] to the unit inputs e = 4 c + l, the planes of every class, the A bytes and the biases"""
    unit = np.zeros((96, 24), dtype=np.uint64)
    for c in range(24):
        for l in range(4):
            unit[4 * c + l, c] = pow(B, l, P)
    U = lfo.crt(unit).reshape(96, 24) % np.uint64(P)
    planes = [[] for _ in range(3)]
    for w in range(24):
        cls = {(e // 4) % 3 for e in range(96) if int(U[e, w])}
        assert len(cls) == 1, f"plane {w} is reached by the classes {cls}"
        planes[cls.pop()].append(w)
    assert all(len(p) == 8 for p in planes)
    A = np.zeros((3, 2, 64, 16), dtype=np.int64)
    for u in range(3):
        for p in range(8):
            for q in range(8):
                for l in range(4):
                    T = int(U[4 * (u + 3 * q) + l, planes[u][p]])
                    v = T - P if T > REACH else T
                    for byte in range(8):
                        d = ((v + 128) % 256) - 128
                        v = (v - d) // 256
                        m = 8 * (p >> 1) + 4 * (p & 1) + (byte & 3)
                        A[u, byte >> 2, 32 * (q >> 2) + m, 4 * (q & 3) + l] = d
                    assert v == 0
    N = 17 * P - 4096 * 0x0101010101010101
    beta = [4096 + ((N >> (8 * b)) & 0xFF if b < 7 else N >> 56) for b in range(8)]
    assert N >= 0 and beta[7] < 4096 + 256 and sum(bb << (8 * b) for b, bb in enumerate(beta)) == 17 * P
    bias = (beta[0] + 256 * beta[1] + 65536 * beta[2], beta[3] + 256 * beta[4] + 65536 * beta[5], beta[6] + 256 * beta[7])
    return planes, A, bias


def _kernel_order(planes, A, bias, v, k):
    """bit-plane k of the entries v [24][NEL][4] as one wave per class computes it: out [NEL][24]"""
    out = np.zeros((NEL, 24), dtype=np.uint64)
    dig = np.sign(v) * ((np.abs(v) >> k) & 1)
    worst = 0
    for u in range(3):
        Bop = np.zeros((64, 16), dtype=np.int64)
        for lane in range(64):
            n, h = lane & 31, lane >> 5
            for jj in range(4):
                Bop[lane, 4 * jj:4 * jj + 4] = dig[u + 3 * (4 * h + jj), n]
        # tile t, row m, column n: A and B meet position by position inside a lane half, summed over both halves
        Cm = [sum(A[u, t, 32 * hh:32 * hh + 32] @ Bop[32 * hh:32 * hh + 32].T for hh in range(2)) for t in range(2)]
        worst = max(worst, max(int(np.abs(c).max()) for c in Cm))
        for n in range(NEL):
            for h in range(2):
                for j in range(4):
                    s = [int(Cm[b >> 2][8 * j + 4 * h + (b & 3), n]) for b in range(8)]
                    X = s[0] + 256 * s[1] + 65536 * s[2] + bias[0]
                    Y = s[3] + 256 * s[4] + 65536 * s[5] + bias[1]
                    Z = s[6] + 256 * s[7] + bias[2]
                    assert 0 <= X < 1 << 30 and 0 <= Y < 1 << 30 and 0 <= Z < 1 << 22
                    T = Y + (Z << 24)
                    assert T < 1 << 47
                    out[n, planes[u][2 * j + h]] = (X + (T << 24)) % P
    return out, worst


def _reference(v, k, B):
    """CRT of the recomposed bit-plane k: lfo elements i L + l hold the digit l of element i"""
    dig = np.sign(v) * ((np.abs(v) >> k) & 1)                      # [24][NEL][4]
    x = np.where(dig < 0, P - 1, dig).astype(np.uint64)            # -1 -> p - 1
    x = np.ascontiguousarray(x.transpose(1, 2, 0)).reshape(NEL * 4, 24)
    return lfo.crt(lfo.recompose(x, B, 4)).reshape(NEL, 24) % np.uint64(P)


@pytest.mark.parametrize("logB", [16, 19])
def test_byte_cut_matrix_is_the_crt_of_the_recomposed_digits(logB):
    B = 1 << logB
    planes, A, bias = _matrix(B)
    assert np.abs(A).max() <= 128 and A.min() >= -128 and A.max() <= 127
    rng = np.random.default_rng(11)
    top = (1 << K) - 1
    cases = {"random": rng.integers(-top, top + 1, size=(24, NEL, 4)), "all +": np.full((24, NEL, 4), top), "all -": np.full((24, NEL, 4), -top),
             "zero": np.zeros((24, NEL, 4), dtype=np.int64)}
    for name, v in cases.items():
        for k in (range(K) if name == "random" else (0, K - 1)):
            got, worst = _kernel_order(planes, A, bias, v, k)
            assert worst <= 32 * 128 <= 32 * 255, f"{name}: a partial sum of {worst}"
            want = _reference(v, k, B)
            assert (got == want).all(), f"B = 2^{logB}, {name}, bit-plane {k}: {int((got != want).sum())} words differ"
    # every digit +-1: a partial sum is the signed sum of a row's 32 bytes -- its bound is met by the row with the largest such sum
    row_sums = np.abs(A.reshape(3, 2, 2, 32, 16).transpose(0, 1, 3, 2, 4).reshape(3, 2, 32, 32).sum(axis=3))
    _, worst = _kernel_order(planes, A, bias, cases["all +"], 0)
    assert worst == row_sums.max() <= 32 * 128
