"""The trailing empty rows of the constraint matrices (csrc/lf_live_rows.h), host side only: the live row count lf_ccs_load keeps and the padded-count schedule of
the linearization rounds, against brute-force models.  The library is reached through its lfdbg_* test hooks (no GPU, no context)."""
import ctypes as C

import numpy as np
import pytest

from latticefold_amd import api

GRANULE, MIN_M = 4096, 1 << 14          # defaults of lf_live_rows.h
GRANULE_LOW, MIN_M_LOW = 8, 16          # LF_LIVE_ROWS_LOW


def _lib():
    L = api._lib()
    L.lfdbg_live_rows_csr.argtypes = [C.c_uint, C.c_size_t, C.POINTER(C.POINTER(C.c_uint32))]
    L.lfdbg_live_rows_csr.restype = C.c_size_t
    L.lfdbg_live_schedule.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_uint, C.POINTER(C.c_size_t)]
    L.lfdbg_live_schedule.restype = None
    return L


def _live_rows(rowptrs, m):
    rp = [np.ascontiguousarray(a, dtype=np.uint32) for a in rowptrs]
    arr = (C.POINTER(C.c_uint32) * len(rp))(*[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in rp])
    return _lib().lfdbg_live_rows_csr(len(rp), m, arr)


def _brute_live_rows(rowptrs, m):
    live = 0
    for rp in rowptrs:
        for r in range(m):
            if rp[r + 1] > rp[r]:
                live = max(live, r + 1)
    return live


def _rowptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def test_live_rows_of_csr():
    rng = np.random.default_rng(7)
    m = 64
    cases = [[np.zeros(m, dtype=int)] * 3]                                  # all matrices empty -> 0
    for last in (0, 1, 2, 3, 5, 7, 8, 9, m // 2 - 1, m // 2, m - 1):
        c = np.zeros(m, dtype=int)
        c[last] = 1
        cases.append([np.zeros(m, dtype=int), c, np.zeros(m, dtype=int)])  # one entry, in the middle matrix only
        full = np.zeros(m, dtype=int)
        full[:last + 1] = 2
        cases.append([full, c, c])
    for _ in range(40):                                                     # gaps anywhere, a different last row per matrix
        t = int(rng.integers(1, 9))
        cs = []
        for _j in range(t):
            c = rng.integers(0, 3, size=m) * (rng.random(m) < 0.3)
            c[int(rng.integers(0, m + 1)):] = 0
            cs.append(c)
        cases.append(cs)
    for cs in cases:
        rps = [_rowptr(c) for c in cs]
        assert _live_rows(rps, m) == _brute_live_rows(rps, m)


def _schedule(m, live, low):
    s = m.bit_length() - 1
    out = (C.c_size_t * s)()
    _lib().lfdbg_live_schedule(m, live, 1 if low else 0, s, out)
    return list(out)


@pytest.mark.parametrize("low", [True, False], ids=["low", "default"])
def test_schedule_against_a_brute_force_model(low):
    """For m = 2^4 .. 2^12 and every live_rows: simulate which entries of every round's tables are written, zeroed or non-zero.
    - a truncated round (fewer live entries than the table has) reads entries [0, 2 e_i) of the previous tables (the fused fix of pair p reads 4p .. 4p+3,
      p < e_i / 2): all of them were written by the previous pass; it covers whole pairs; the counts halve exactly (no ceilings);
    - every entry that can be non-zero (row < live_rows in round 1, pairs with a non-zero member afterwards) lies in the live prefix;
    - once a round runs whole (after ONE zero-fill of the rest) every later round does; the counts never exceed the table;
    - live = m, and any prefix above m / 2 or below the size threshold, reproduces today's whole-table counts."""
    g, min_m = (GRANULE_LOW, MIN_M_LOW) if low else (GRANULE, MIN_M)
    for s in list(range(4, 13)) + ([] if low else [14, 15]):
        m = 1 << s
        whole = [m >> i for i in range(s)]
        # (above 2^12, where the default threshold starts: a stride plus the boundaries)
        lives = range(m + 1) if s <= 12 else sorted(set(range(0, m + 1, 61)) | {x + dx for x in (0, g, m // 4, m // 2, m) for dx in (-1, 0, 1) if 0 <= x + dx <= m})
        for live in lives:
            e = _schedule(m, live, low)
            pad = max(g, -(-live // g) * g)
            if m < min_m or pad > m // 2:
                assert e == whole, (m, live, e)
                continue
            assert e[0] == pad and e[0] >= live and e[0] % 2 == 0, (m, live, e)
            written, support, n, zero_fills = e[0], live, m, 0
            for i in range(1, s):                       # round i + 1 from the tables of round i
                n_new, support = n // 2, -(-support // 2)
                assert e[i] <= n_new and support <= e[i], (m, live, i, e)
                if e[i] < n_new:                        # truncated round
                    assert written < n, (m, live, i, e)                       # (never back to a prefix once whole)
                    assert 2 * e[i] == written and e[i] % 2 == 0, (m, live, i, e)
                else:
                    if written < n:
                        zero_fills += 1                 # the driver zeroes [written, n) of the previous tables: whole from here on
                    assert e[i] == n_new
                written, n = e[i], n_new
            assert zero_fills == 1, (m, live, e)
            # a granule of 2^k gives at least k rounds on the prefix
            assert sum(1 for i in range(s) if e[i] < (m >> i)) >= min(g.bit_length() - 1, s - 1), (m, live, e)
    assert _schedule(1 << 20, (1 << 18) + 2, False)[:3] == [(1 << 18) + 4096, (1 << 17) + 2048, (1 << 16) + 1024]
