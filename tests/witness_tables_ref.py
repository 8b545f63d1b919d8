"""numpy restatements and shapes shared by test_witness_tables_cpu.py and test_gpu_witness_tables.py: the witness tables of include/lfhip_tables.h (f-hat,
z, M z, M^T v, fix_variables on tables).  Not a test module.

Everything here is arithmetic on canonical residues: slot-wise ring products through workload.ring_mul_ntt, sums in Python integers (object dtype) mod p."""
import numpy as np

from latticefold_amd.workload import RINGS, make_workload, ring_mul_ntt, splitmix_fq

# the two constants of lf_spmv_t's heavy-column path, as latticefold_amd/csrc/lf_spmv_t_plan.h defines them (SPMV_T_HEAVY, SPMV_T_CHUNK): a column of at
# least HEAVY entries leaves the one-thread-per-(column, slot) path and is cut into work items of at most CHUNK entries
SPMV_T_HEAVY = 64
SPMV_T_CHUNK = 512

NEW_SYMBOLS = ("lf_witness_get_fhat", "lf_witness_get_fhat_device", "lf_witness_get_z", "lf_witness_get_z_device", "lf_witness_mz", "lf_witness_mz_device",
               "lf_spmv_t", "lf_spmv_t_device", "lf_mle_fix_variables", "lf_mle_fix_variables_device")


def oracle_for(ring):
    if ring == "babybear":
        import lfo_bb
        return lfo_bb
    import lfo
    return lfo


def workload(name, ccs="r1cs", l=1):
    if ccs == "general5":
        from test_gpu_wide_ccs import general_deg5
        return general_deg5(name)
    return make_workload(name, 0, ccs=ccs, l=l)


def rand_ring(seed, n, wl):
    """n ring elements with eight different slots"""
    return splitmix_fq(seed, 0, n * wl.RE, wl.ring).reshape(n, wl.RE)


def embed(ch):
    """F_{p^tau} element (tau words) -> the slot-constant ring element"""
    return np.tile(np.asarray(ch, dtype=np.uint64), 8)


def add_mod(a, b, p):
    return ((a.astype(object) + b.astype(object)) % p).astype(np.uint64)


def sub_mod(a, b, p):
    return ((a.astype(object) - b.astype(object)) % p).astype(np.uint64)


def sum_mod(a, p):
    """sum over axis 0"""
    return (a.astype(object).sum(axis=0) % p).astype(np.uint64)


def fhat_np(f_coeff, wl):
    """Witness::get_fhat by the formula of include/lfhip_tables.h: (tau, m, RE); tab_j[:N, 0::tau] = f_coeff[:, 8 j : 8 j + 8], zero elsewhere"""
    f = np.asarray(f_coeff, dtype=np.uint64).reshape(wl.N, wl.RE)
    out = np.zeros((wl.tau, wl.m, wl.RE), dtype=np.uint64)
    for j in range(wl.tau):
        out[j, :wl.N, 0::wl.tau] = f[:, 8 * j:8 * j + 8]
    return out


def csr_entries(rowptr, col, val, RE):
    """(rows, cols, vals) of the entries of a CSR matrix"""
    rp = np.asarray(rowptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return rows, np.asarray(col, dtype=np.int64)[:len(rows)], np.asarray(val, dtype=np.uint64).reshape(-1, RE)[:len(rows)]


def spmv_np(rowptr, col, val, z, m, ring):
    """M z: (m, RE)"""
    p, RE, _ = RINGS[ring]
    rows, cols, vals = csr_entries(rowptr, col, val, RE)
    out = np.zeros((m, RE), dtype=object)
    if len(rows):
        np.add.at(out, rows, ring_mul_ntt(vals, z[cols], ring).astype(object))
    return (out % p).astype(np.uint64)


def spmv_t_np(rowptr, col, val, v, n, ring):
    """M^T v as a scatter-add over the entries: out[c] += M[r][c] (.) v[r]; (n, RE)"""
    p, RE, _ = RINGS[ring]
    rows, cols, vals = csr_entries(rowptr, col, val, RE)
    out = np.zeros((n, RE), dtype=object)
    if len(rows):
        np.add.at(out, cols, ring_mul_ntt(vals, v[rows], ring).astype(object))
    return (out % p).astype(np.uint64)


def inner_np(a, b, ring):
    """sum_i a[i] (.) b[i]: one ring element"""
    return sum_mod(ring_mul_ntt(a, b, ring), RINGS[ring][0])


def fix_np(tab, r, ring):
    """DenseMultilinearExtension::fix_variables of the LOWEST variable at the ring element r (a slot-constant embedding of a challenge):
    new[j] = old[2j] + r (old[2j+1] - old[2j]); tab (..., len, RE)"""
    p = RINGS[ring][0]
    lo, hi = tab[..., 0::2, :], tab[..., 1::2, :]
    return add_mod(lo, ring_mul_ntt(sub_mod(hi, lo, p), r, ring), p)


def csr_from_columns(counts, m, n, wl, seed):
    """a matrix of m rows and n columns whose column c holds counts[c] entries, at rows 0 .. counts[c] - 1 shifted by c (so neighbouring heavy columns share
    rows), random ring-valued entries: CSR (rowptr, col, val)"""
    ent = [((c + i) % m, c) for c in range(n) for i in range(int(counts[c]))]
    ent.sort()
    rows = np.array([e[0] for e in ent], dtype=np.int64)
    cols = np.array([e[1] for e in ent], dtype=np.uint32)
    rowptr = np.zeros(m + 1, dtype=np.uint32)
    if len(ent):
        np.add.at(rowptr, rows + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.uint32)
    val = rand_ring(seed, max(len(ent), 1), wl)[:len(ent)]
    return rowptr, cols, val


def lcccs_parts(lcccs, wl):
    """the flat LCCCS r[s] v[tau] cm[kappa] u[t] x_w[l] h -> (r, v, u)"""
    a = np.asarray(lcccs, dtype=np.uint64).reshape(-1, wl.RE)
    s, tau, kap, t = wl.s, wl.tau, wl.kappa, wl.t
    return a[:s], a[s:s + tau], a[s + tau + kap:s + tau + kap + t]
