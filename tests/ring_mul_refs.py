"""References for products of arrays of ring elements (tests/test_gpu_ring_mul.py, tests/test_ring_mul_cpu.py), none of them the code under test: the numpy
schoolbook of latticefold_amd.workload, Python integers per slot (field_corners.Ref), and big-integer polynomial products mod the cyclotomic polynomial."""
import numpy as np

import field_corners as fc
from latticefold_amd.workload import RINGS, _fp_add, ring_mul_ntt


def ntt_sum_numpy(a, b, ring):
    """sum over the leading axis of the slot-wise products, through workload.ring_mul_ntt and _fp_add"""
    acc = ring_mul_ntt(a[0], b[0], ring)
    for i in range(1, a.shape[0]):
        acc = _fp_add(acc, ring_mul_ntt(a[i], b[i], ring), ring)
    return acc


def ntt_sum_bigint(a, b, ring):
    """the same in Python integers: per slot F_p[Y]/(Y^tau - nu), nu = default_nonres(ring) (field_corners.Ref)"""
    ref = fc.Ref(ring)
    A, B = fc.elems(a, ring), fc.elems(b, ring)
    out = []
    for x in range(a.shape[1]):
        acc = ref.rzero()
        for i in range(a.shape[0]):
            acc = ref.radd(acc, ref.rmul(A[i][x], B[i][x]))
        out.append(acc)
    return fc.pack(out)


def coeff_sum_bigint(a, b, ring):
    """sum_i a_i[x] * b_i[x] in Z_p[X]/(X^d - X^(d/2) + 1): integer schoolbook products, X^k = X^(k - d/2) - X^(k - d) from the top down, then mod p"""
    p, d, _tau = RINGS[ring]
    out = np.zeros((a.shape[1], d), dtype=np.uint64)
    A, B = a.astype(object), b.astype(object)
    for x in range(a.shape[1]):
        c = np.zeros(2 * d - 1, dtype=object)
        for i in range(a.shape[0]):
            for k in range(d):
                c[k:k + d] += A[i, x, k] * B[i, x]
        for k in range(2 * d - 2, d - 1, -1):
            c[k - d // 2] += c[k]
            c[k - d] -= c[k]
        out[x] = [int(v) % p for v in c[:d]]
    return out
