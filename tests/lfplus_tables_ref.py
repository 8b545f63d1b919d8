"""Python-integer references of the LatticeFold+ table calls (tests/test_lfplus_tables_cpu.py, tests/test_gpu_lfplus_tables.py): none of it the code under test.
eq is the product formula, an evaluation the weighted sum, fix_variables the weighted sum over the entries below an output, M^T v the transposed loop over the
CSR entries; ring products are lfplus_mlsumcheck_ref.rmul (Python integers in numpy object arrays)."""
import numpy as np

import lfplus_mlsumcheck_ref as ref

P, D = ref.P, ref.D


def eq_weights(r):
    """[eq(r, x) for x < 2^len(r)] as Python integers by the product formula, bit i of x paired with r[i]"""
    out = []
    for x in range(1 << len(r)):
        w = 1
        for i, ri in enumerate(r):
            ri = int(ri)
            w = w * (ri if (x >> i) & 1 else (1 - ri) % P) % P
        out.append(w)
    return out


def eq_words(r):
    return np.array(eq_weights(r), dtype=object).astype(np.uint64)


def py_eval(tables, length, r):
    """out[j] = sum_{x < length} eq(r, x) tables[j][x]: tables (T, >= length, 16) -> (T, 16)"""
    w = np.array(eq_weights(r)[:length], dtype=object)
    t = np.asarray(tables).astype(object)[:, :length]
    return ((t * w[None, :, None]).sum(axis=1) % P).astype(np.uint64)


def py_fix(tables, r):
    """the lowest len(r) variables of tables (T, 2^nv, 16) fixed at r -> (T, 2^nv >> len(r), 16)"""
    w = np.array(eq_weights(r), dtype=object)
    t = np.asarray(tables).astype(object)
    t = t.reshape(t.shape[0], -1, w.size, D)
    return ((t * w[None, None, :, None]).sum(axis=2) % P).astype(np.uint64)


def py_spmv_t(mat, v):
    """out[c] = sum over the entries (r, c) of M[r][c] * v[r], in the order the CSR lists them"""
    rowptr, col, val = mat
    n = rowptr.size - 1
    out = np.zeros((n, D), dtype=object)
    if col.size:
        rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
        prod = ref.rmul(val, np.asarray(v)[rows])                                # one product per entry, (nnz, 16)
        for k in range(col.size):
            out[col[k]] = out[col[k]] + prod[k]
    return (out % P).astype(np.uint64)


def ring_dot(a, b):
    """sum_x a[x] * b[x] in the ring, (n, 16) x (n, 16) -> (16,)"""
    return (ref.rmul(a, b).sum(axis=0) % P).astype(np.uint64)
