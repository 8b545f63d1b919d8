// lfp_digits.cpp -- host bodies of the "gadget maps on arrays" section of include/lfplus.h: lfplus_balanced_decompose, lfplus_balanced_recompose, lfplus_linf_norm,
// their _device forms and lfplus_set_matrices_gadget (kernels: lfp_digits.hip).  One body per call for both memory spaces, as lfp_tables.cpp: a host array is staged
// through the context's pooled scratch, a device array is read and written in place.
//   Nothing resident is read or written by the three array calls: the buffers are the call's own blocks of the pool (given back before it returns), the work runs
// on the context's first stream, and neither the witness, the from_f results, a pass pending on the second stream nor the state of a generic sumcheck is looked at.
// lfplus_set_matrices_gadget replaces the resident matrices only after the new set is complete: every refusal and every failure leaves the previous set resident.
//   The refusals come in the order lfplus.h states them; every one before the word test of the O(n) input leaves before anything is allocated or enqueued.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lfp_array_call.h"
#include "lfp_ctx.h"
#include "lfp_guard.h"
#include "lf_dev_ptr.h"

using lfdev::Origin;
using namespace lfp_arr;

namespace {
u32 block_cap() {
    const char *e = getenv("LFPLUS_DIGIT_BLOCKS");   // workgroups of lfplus_balanced_decompose / lfplus_balanced_recompose at most (default 2048: 8 per CU); read once per call
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= 65535 ? (u32)v : 2048u;
}
// b^i 2^64 mod p for i < k: the k powers, computed once
lfp::DigitPows digit_pows(u64 b, u32 k) {
    lfp::DigitPows pw;
    memset(&pw, 0, sizeof(pw));
    u64 cur = 1;
    for (u32 i = 0; i < k; i++) {
        pw.pM[i] = to_mont(cur);
        cur = (u64)((unsigned __int128)cur * (b % lfp::P) % lfp::P);
    }
    return pw;
}
const char *const ENVELOPE = ": outside the envelope (1 <= count, count * k <= 2^28, 1 <= k <= 64, 2 <= b <= 2^62, layout 0 or 1)";

// decompose: in count elements -> out count * k; recompose: in count * k -> out count
int digits_impl(lfplus_ctx *c, const uint64_t *in, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out, bool recompose, Origin o, const char *who) {
    const std::string w(who);
    if (!in || !out) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (k < 1 || k > 64 || count < 1 || count > (1ull << 28) / k || b < 2 || b > (1ull << 62) || (layout != 0 && layout != 1)) return fail(c, LFPLUS_E_ARG, w + ENVELOPE);
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const bool dev = o == Origin::device;
    const u64 nin = recompose ? count * k : count, nout = recompose ? count : count * k, ibytes = nin * 128, obytes = nout * 128;
    if (ranges_overlap(out, obytes, in, ibytes)) return fail(c, LFPLUS_E_ARG, w + ": out overlaps in (the map permutes)");
    if (dev && (lfp_dev_ptr_check(c, in, nin, who) || lfp_dev_ptr_check(c, out, nout, who))) return LFPLUS_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const u64 *din = in;
    u64 *dout = out, *tin = nullptr;
    u32 *dflag = nullptr;
    bool ok = sc.get(&dflag, 8);
    if (ok && !dev) ok = sc.get(&tin, ibytes) && sc.get(&dout, obytes);
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    hipError_t e = hipMemsetAsync(dflag, 0, 4, c->st);
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(tin, in, ibytes, hipMemcpyHostToDevice, c->st);
        din = tin;
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    const u32 blocks = lfp::digit_blocks(count * 16, block_cap());
    if (recompose) lfp::launch_digits_recompose(din, count, k, layout, digit_pows(b, k), dout, dflag, blocks, c->st);
    else lfp::launch_digits_decompose(din, count, b, k, layout, dout, dflag, blocks, c->st);
    u32 flag = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (flag) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in in");
    if (!dev) {
        e = hipMemcpyAsync(out, dout, obytes, hipMemcpyDeviceToHost, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) return hip_fail(c, w, e);
    }
    return LFPLUS_OK;
}

int linf_impl(lfplus_ctx *c, const uint64_t *v, uint64_t count, uint64_t *absmax, Origin o, const char *who) {
    const std::string w(who);
    if (!v || !absmax) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (count < 1 || count > (1ull << 28)) return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= count <= 2^28)");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const bool dev = o == Origin::device;
    const u64 bytes = count * 128;
    if (!dev && ranges_overlap(absmax, 8, v, bytes)) return fail(c, LFPLUS_E_ARG, w + ": absmax overlaps v");
    if (dev && lfp_dev_ptr_check(c, v, count, who)) return LFPLUS_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const u64 *dv = v;
    u64 *tv = nullptr, *res = nullptr;      // res: the maximum, then the word flag
    bool ok = sc.get(&res, 16);
    if (ok && !dev) ok = sc.get(&tv, bytes);
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    hipError_t e = hipMemsetAsync(res, 0, 16, c->st);
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(tv, v, bytes, hipMemcpyHostToDevice, c->st);
        dv = tv;
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    lfp::launch_absmax(dv, (size_t)count * 16, res, c->st, (u32 *)(res + 1));
    u64 h[2] = {0, 0};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (h[1]) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in v");
    *absmax = h[0];
    return LFPLUS_OK;
}

// one short matrix (rows x m, validated as lfp_upload_matrix validates its n x n one) -> the complete n x n LfpMatrix of its gadget form, expanded on the device
int upload_gadget(lfplus_ctx *c, u64 rows, u64 m, u64 n, u32 k, const lfp::DigitPows &pw, const u32 *rowptr, const u32 *col, const u64 *val, LfpMatrix &mx) {
    if (!rowptr || !col || !val || rowptr[0] != 0) return fail(c, LFPLUS_E_ARG, "lfplus_set_matrices_gadget: matrix: null / malformed CSR");
    for (u64 r = 0; r < rows; r++) if (rowptr[r + 1] < rowptr[r]) return fail(c, LFPLUS_E_ARG, "lfplus_set_matrices_gadget: matrix: rowptr not monotone");
    const u64 nnz = rowptr[rows];
    if (nnz * k >= (1ull << 32)) return fail(c, LFPLUS_E_ARG, "lfplus_set_matrices_gadget: matrix: nnz * k must stay below 2^32");
    std::vector<u32> cp(m + 1, 0);
    for (u64 e = 0; e < nnz; e++) {
        if (col[e] >= m) return fail(c, LFPLUS_E_ARG, "lfplus_set_matrices_gadget: matrix: column index out of range");
        cp[(size_t)col[e] + 1]++;
    }
    if (!canonical(val, nnz * 16)) return fail(c, LFPLUS_E_ARG, "lfplus_set_matrices_gadget: matrix: non-canonical word");
    for (u64 j = 0; j < m; j++) cp[j + 1] += cp[j];
    // c b^i is a constant polynomial exactly when c is: decided on the short values
    bool const_coef = true;
    for (u64 e = 0; e < nnz && const_coef; e++)
        for (int t = 1; t < 16; t++) if (val[e * 16 + t]) { const_coef = false; break; }
    const u64 big = nnz * k;
    mx.nnz = (size_t)big;
    mx.const_coef = const_coef;
    const size_t vb = (size_t)(big ? big : 1) * 128, ib = (size_t)(big ? big : 1) * 4;
    if (lfp_dev_malloc(&mx.rowptr, (n + 1) * 4) != hipSuccess || lfp_dev_malloc(&mx.col, ib) != hipSuccess || lfp_dev_malloc(&mx.valM, vb) != hipSuccess ||
        lfp_dev_malloc(&mx.colptr, (n + 1) * 4) != hipSuccess || lfp_dev_malloc(&mx.rowidx, ib) != hipSuccess || lfp_dev_malloc(&mx.valT, vb) != hipSuccess ||
        (const_coef && (lfp_dev_malloc(&mx.valMc, ib * 2) != hipSuccess || lfp_dev_malloc(&mx.valTc, ib * 2) != hipSuccess)))
        return fail(c, LFPLUS_E_HIP, "lfplus_set_matrices_gadget: hipMalloc (matrix)");
    // the short arrays and the short column counts (as pointers) are all that crosses PCIe
    Scratch sc(c);
    u32 *rp_s = nullptr, *col_s = nullptr, *cp_s = nullptr, *perm = nullptr;
    u64 *val_s = nullptr;
    void *tmp = nullptr;
    const size_t tmp_bytes = nnz ? lfp::gadget_perm_bytes(nnz, m) : 8;
    if (!sc.get(&rp_s, (rows + 1) * 4) || !sc.get(&cp_s, (m + 1) * 4) || !sc.get(&col_s, (nnz ? nnz : 1) * 4) || !sc.get(&val_s, (nnz ? nnz : 1) * 128) ||
        !sc.get(&perm, (nnz ? nnz : 1) * 4) || !sc.get(&tmp, tmp_bytes))
        return fail(c, LFPLUS_E_HIP, "lfplus_set_matrices_gadget: out of device memory");
    const std::string w("lfplus_set_matrices_gadget");
    hipError_t e = hipMemcpyAsync(rp_s, rowptr, (rows + 1) * 4, hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess) e = hipMemcpyAsync(cp_s, cp.data(), (m + 1) * 4, hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(col_s, col, nnz * 4, hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(val_s, val, nnz * 128, hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess && nnz) e = lfp::launch_gadget_perm(col_s, nnz, m, perm, tmp, tmp_bytes, c->st);
    if (e != hipSuccess) return hip_fail(c, w, e);
    const lfp::GadgetOut go = {mx.rowptr, mx.col, mx.colptr, mx.rowidx, mx.valM, mx.valT, mx.valMc, mx.valTc};
    lfp::launch_gadget_expand(rp_s, col_s, val_s, cp_s, perm, rows, m, n, nnz, k, pw, go, c->st);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);      // the host staging vector and the scratch die here
    if (e != hipSuccess) return hip_fail(c, w, e);
    return LFPLUS_OK;
}

int set_gadget_impl(lfplus_ctx *c, uint64_t rows, uint64_t m, uint64_t b, uint32_t k, uint64_t n, uint32_t nM, const uint32_t *const *rowptr, const uint32_t *const *col,
                    const uint64_t *const *val) {
    const std::string w("lfplus_set_matrices_gadget");
    if (nM && (!rowptr || !col || !val)) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (!n || n > (1ull << 32) || nM > 64 || rows > n || k < 1 || k > 64 || b < 2 || b > (1ull << 62) || !m || m > n || m * k != n)
        return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= n <= 2^32, nM <= 64, rows <= n, m * k == n, 1 <= k <= 64, 2 <= b <= 2^62)");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    HIPCHK(c, hipSetDevice(c->device));
    const lfp::DigitPows pw = digit_pows(b, k);
    std::vector<LfpMatrix> fresh(nM);
    for (u32 q = 0; q < nM; q++) {
        const int rc = upload_gadget(c, rows, m, n, k, pw, rowptr[q], col[q], val[q], fresh[q]);
        if (rc) { for (LfpMatrix &x : fresh) x.release(); return rc; }
    }
    auto owner = std::make_shared<lfplus_ctx::MatsOwner>();
    owner->m = fresh;      // the owner releases the device arrays with its last holder; c->mats is the view the kernels take
    c->drop_mats();
    c->mats_ref = owner;
    c->mats.swap(fresh);
    c->mats_n = n;
    return LFPLUS_OK;
}
}  // namespace

// a NULL context is LFPLUS_E_ARG before any device is touched: the answer on a machine without a GPU as well
extern "C" int lfplus_balanced_decompose(lfplus_ctx *c, const uint64_t *in, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(digits_impl(c, in, count, b, k, layout, out, false, Origin::host, "lfplus_balanced_decompose"), oom(c, "lfplus_balanced_decompose: out of host memory"))
}
extern "C" int lfplus_balanced_decompose_device(lfplus_ctx *c, const uint64_t *in, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(digits_impl(c, in, count, b, k, layout, out, false, Origin::device, "lfplus_balanced_decompose_device"),
              oom(c, "lfplus_balanced_decompose_device: out of host memory"))
}
extern "C" int lfplus_balanced_recompose(lfplus_ctx *c, const uint64_t *in, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(digits_impl(c, in, count, b, k, layout, out, true, Origin::host, "lfplus_balanced_recompose"), oom(c, "lfplus_balanced_recompose: out of host memory"))
}
extern "C" int lfplus_balanced_recompose_device(lfplus_ctx *c, const uint64_t *in, uint64_t count, uint64_t b, uint32_t k, int layout, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(digits_impl(c, in, count, b, k, layout, out, true, Origin::device, "lfplus_balanced_recompose_device"),
              oom(c, "lfplus_balanced_recompose_device: out of host memory"))
}
extern "C" int lfplus_linf_norm(lfplus_ctx *c, const uint64_t *v, uint64_t count, uint64_t *absmax) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(linf_impl(c, v, count, absmax, Origin::host, "lfplus_linf_norm"), oom(c, "lfplus_linf_norm: out of host memory"))
}
extern "C" int lfplus_linf_norm_device(lfplus_ctx *c, const uint64_t *v, uint64_t count, uint64_t *absmax) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(linf_impl(c, v, count, absmax, Origin::device, "lfplus_linf_norm_device"), oom(c, "lfplus_linf_norm_device: out of host memory"))
}
extern "C" int lfplus_set_matrices_gadget(lfplus_ctx *c, uint64_t rows, uint64_t m, uint64_t b, uint32_t k, uint64_t n, uint32_t nM, const uint32_t *const *rowptr,
                                          const uint32_t *const *col, const uint64_t *const *val) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(set_gadget_impl(c, rows, m, b, k, n, nM, rowptr, col, val), oom(c, "lfplus_set_matrices_gadget: out of host memory"))
}
