"""The int8 matrix of compute_f_0 (csrc/lf_fold_i8.hip) on integers, without a GPU: the wrap X^24 = X^12 - 1 built into the matrix of the challenges,
restated in numpy in the kernel's operand order -- A words [row tile][K-step][lane][16], B bytes = the 16 digits of one plane entry per lane group and K-step,
C register r of lane (n, g) = row 4 g + r, column n -- against the polynomial products sum_i rho_i * digit-plane_i mod X^24 - X^12 + 1."""
import numpy as np

K = 16


def _wrapped_matrix(rho):
    """W [24][side][a][k] as the kernel forms it from rho [2][K][24]"""
    W = np.zeros((24, 2, 24, K), dtype=np.int64)
    at = lambda r, i: int(r[i]) if 0 <= i < 24 else 0
    for side in range(2):
        for k in range(K):
            r = rho[side, k]
            for c in range(24):
                for a in range(24):
                    W[c, side, a, k] = at(r, c - a) - at(r, c + 24 - a) - at(r, c + 36 - a) if c < 12 else at(r, c - a) + at(r, c + 12 - a)
    return W


def _reference(rho, v):
    """f_0 [24] of one column: v [2][24] plane entries, digit_k(v) = sign(v) bit_k(|v|); products reduced with X^24 = X^12 - 1 top down"""
    u = np.zeros(47, dtype=np.int64)
    for side in range(2):
        for k in range(K):
            d = np.sign(v[side]) * ((np.abs(v[side]) >> k) & 1)
            u += np.convolve(rho[side, k].astype(np.int64), d)
    for p in range(46, 23, -1):
        u[p - 12] += u[p]
        u[p - 24] -= u[p]
    return u[:24]


def _kernel_order(W, v):
    """the MFMA steps of one 16-column tile whose columns all hold v: A[mt][s][lane][e], B[s][lane][e], sum over (s, g, e) with A and B taken position by position"""
    A = np.zeros((2, 12, 64, 16), dtype=np.int64)
    B = np.zeros((12, 64, 16), dtype=np.int64)
    for s in range(12):
        for lane in range(64):
            m, g = lane & 15, lane >> 4
            side, a = divmod(4 * s + g, 24)
            x = int(v[side, a])
            B[s, lane] = [(-1 if x < 0 else 1) * ((abs(x) >> e) & 1) for e in range(16)]
            for mt in range(2):
                if 16 * mt + m < 24:
                    A[mt, s, lane] = W[16 * mt + m, side, a]
    assert np.abs(A).max() <= 127
    out = np.zeros(24, dtype=np.int64)
    for mt in range(2):
        for g in range(4):
            for r in range(4):
                c = 16 * mt + 4 * g + r
                if c < 24:
                    # element (row 4 g + r, column n) of the tile: the rows of A with m = 4 g + r against the column's lanes, over all four lane groups
                    out[c] = sum(int(A[mt, s, 16 * gg + 4 * g + r] @ B[s, 16 * gg + 0]) for s in range(12) for gg in range(4))
    return out


def test_wrapped_matrix_is_the_product_mod_phi72():
    rng = np.random.default_rng(7)
    for trial in range(4):
        rho = rng.integers(-32, 32, size=(2, K, 24))
        if trial == 1:
            rho[:] = -32                                   # every entry of W at its bound
        if trial == 2:
            rho[1, K - 1] = 0
            rho[1, K - 1, 0] = 1                           # the constant ONE comes last (get_rhos)
        W = _wrapped_matrix(rho)
        assert np.abs(W).max() <= 64                       # at most two challenge coefficients meet in an entry: int8
        vs = [rng.integers(-(1 << 15) + 1, 1 << 15, size=(2, 24)), np.full((2, 24), (1 << 15) - 1), np.full((2, 24), -((1 << 15) - 1)), np.zeros((2, 24), dtype=np.int64),
              np.full((2, 24), (1 << 16) - 1)]
        one = np.zeros((2, 24), dtype=np.int64)
        one[1, 23] = -1
        for v in vs + [one]:
            want = _reference(rho, v)
            got = np.einsum("csak,sak->c", W, np.sign(v)[:, :, None] * ((np.abs(v)[:, :, None] >> np.arange(K)) & 1))
            assert (got == want).all()
            assert np.abs(got).max() <= 768 * 64
            if trial == 0:
                assert (_kernel_order(W, v) == want).all()
