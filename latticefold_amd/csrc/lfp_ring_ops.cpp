// lfp_ring_ops.cpp -- host bodies of the "ring arithmetic on arrays" section of include/lfplus.h: lfplus_ring_mul / lfplus_ring_mul_device (kernel:
// lfp_ring_ops.hip) and lfplus_spmv / lfplus_spmv_device (the slice's launch_spmv_ring on the resident matrices, behind argument checks and the canonical test of
// x).  One body per call for both memory spaces: a host array is staged through the context's pooled scratch, a device array is read and written in place.
//   Nothing resident is read or written: the buffers are the call's own blocks of the pool (given back before it returns), the work runs on the context's first
// stream, and neither the witness, the from_f results, a pass pending on the second stream nor the state of a generic sumcheck is looked at.
//   The refusals come in the order lfplus.h states them; every one before the word test leaves before anything is allocated or enqueued.
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
    const char *e = getenv("LFPLUS_RING_BLOCKS");   // workgroups of lfplus_ring_mul at most (default 2048: 8 per CU); read once per call
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= 65535 ? (u32)v : 2048u;
}

int ring_mul_impl(lfplus_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t n_terms, uint64_t count, int mode, uint64_t *out, Origin o, const char *who) {
    const std::string w(who);
    if (!a || !b || !out) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (n_terms < 1 || n_terms > 64 || count < 1 || count > (1ull << 28) || (mode != LFPLUS_MUL_ELEMENTWISE && mode != LFPLUS_MUL_BROADCAST))
        return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= n_terms <= 64, 1 <= count <= 2^28, mode 0 or 1)");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const bool dev = o == Origin::device;
    const u64 abytes = n_terms * count * 128, bbytes = mode ? n_terms * 128 : abytes, obytes = count * 128;
    const bool b_same_space = !(dev && mode);      // (the coefficients of a broadcast stay on the host: they share no address space with a device `out`)
    const bool in_place_a = out == a && n_terms == 1, in_place_b = out == b && n_terms == 1 && !mode;
    if ((!in_place_a && ranges_overlap(out, obytes, a, abytes)) || (b_same_space && !in_place_b && ranges_overlap(out, obytes, b, bbytes)))
        return fail(c, LFPLUS_E_ARG, w + ": out overlaps an input (it may be exactly a, or exactly b in mode 0, when n_terms == 1)");
    if (dev) {
        if (lfp_dev_ptr_check(c, a, n_terms * count, who)) return LFPLUS_E_ARG;
        if (!mode && lfp_dev_ptr_check(c, b, n_terms * count, who)) return LFPLUS_E_ARG;
        if (lfp_dev_ptr_check(c, out, count, who)) return LFPLUS_E_ARG;
    }
    if (mode && !canonical(b, (size_t)n_terms * 16)) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in b");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const u64 *da = a, *db = b;
    u64 *dout = out, *ta = nullptr, *tb = nullptr, *bM = nullptr;
    u32 *dflag = nullptr;
    bool ok = sc.get(&dflag, 8);
    if (ok && mode) ok = sc.get(&bM, bbytes);
    if (ok && !dev) {
        ok = sc.get(&ta, abytes) && sc.get(&dout, obytes);
        if (ok && !mode && b != a) ok = sc.get(&tb, abytes);      // (a square is uploaded once)
    }
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    std::vector<u64> hbM;
    hipError_t e = hipMemsetAsync(dflag, 0, 4, c->st);
    if (e == hipSuccess && mode) {
        hbM.resize((size_t)n_terms * 16);
        for (size_t i = 0; i < hbM.size(); i++) hbM[i] = to_mont(b[i]);
        e = hipMemcpyAsync(bM, hbM.data(), bbytes, hipMemcpyHostToDevice, c->st);
        db = bM;
    }
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(ta, a, abytes, hipMemcpyHostToDevice, c->st);
        da = ta;
        if (!mode) {
            if (e == hipSuccess && tb) e = hipMemcpyAsync(tb, b, abytes, hipMemcpyHostToDevice, c->st);
            db = tb ? tb : ta;
        }
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    lfp::launch_ring_mul(da, db, (u32)n_terms, count, mode, dout, dflag, lfp::ring_mul_blocks(count, block_cap()), c->st);
    e = hipGetLastError();
    u32 flag = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (flag) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in " + (mode ? "a" : "a or b"));
    if (!dev) {
        e = hipMemcpyAsync(out, dout, obytes, hipMemcpyDeviceToHost, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) return hip_fail(c, w, e);
    }
    return LFPLUS_OK;
}

int spmv_impl(lfplus_ctx *c, uint32_t j, const uint64_t *x, uint64_t n, uint64_t *y, Origin o, const char *who) {
    const std::string w(who);
    if (!x || !y) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (c->mats.empty()) return fail(c, LFPLUS_E_ARG, w + ": no resident matrices (lfplus_set_matrices / lfplus_share_matrices)");
    if (j >= c->mats.size()) return fail(c, LFPLUS_E_ARG, w + ": matrix " + std::to_string(j) + " of " + std::to_string(c->mats.size()));
    if (n != c->mats_n) return fail(c, LFPLUS_E_ARG, w + ": n = " + std::to_string(n) + ", the resident matrices are " + std::to_string(c->mats_n) + " wide");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const u64 bytes = n * 128;
    if (ranges_overlap(x, bytes, y, bytes)) return fail(c, LFPLUS_E_ARG, w + ": y overlaps x (the product gathers)");
    const bool dev = o == Origin::device;
    if (dev && (lfp_dev_ptr_check(c, x, n, who) || lfp_dev_ptr_check(c, y, n, who))) return LFPLUS_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const u64 *dx = x;
    u64 *dy = y, *tx = nullptr;
    u32 *dflag = nullptr;
    bool ok = sc.get(&dflag, 8);
    if (ok && !dev) ok = sc.get(&tx, bytes) && sc.get(&dy, bytes);
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    hipError_t e = hipMemsetAsync(dflag, 0, 4, c->st);
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(tx, x, bytes, hipMemcpyHostToDevice, c->st);
        dx = tx;
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    const LfpMatrix &m = c->mats[j];
    lfp::launch_check_canonical(dx, (size_t)n * 16, dflag, 1u, c->st);
    lfp::launch_spmv_ring(m.rowptr, m.col, m.spmv_vals(), dx, (size_t)n, dy, c->st, m.const_coef);      // (column indices were validated when the matrix was uploaded)
    e = hipGetLastError();
    u32 flag = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (flag) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in x");
    if (!dev) {
        e = hipMemcpyAsync(y, dy, bytes, hipMemcpyDeviceToHost, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) return hip_fail(c, w, e);
    }
    return LFPLUS_OK;
}
}  // namespace

// a NULL context is LFPLUS_E_ARG before any device is touched: the answer on a machine without a GPU as well
extern "C" int lfplus_ring_mul(lfplus_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t n_terms, uint64_t count, int mode, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(ring_mul_impl(c, a, b, n_terms, count, mode, out, Origin::host, "lfplus_ring_mul"), oom(c, "lfplus_ring_mul: out of host memory"))
}
extern "C" int lfplus_ring_mul_device(lfplus_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t n_terms, uint64_t count, int mode, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(ring_mul_impl(c, a, b, n_terms, count, mode, out, Origin::device, "lfplus_ring_mul_device"), oom(c, "lfplus_ring_mul_device: out of host memory"))
}
extern "C" int lfplus_spmv(lfplus_ctx *c, uint32_t j, const uint64_t *x, uint64_t n, uint64_t *y) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(spmv_impl(c, j, x, n, y, Origin::host, "lfplus_spmv"), oom(c, "lfplus_spmv: out of host memory"))
}
extern "C" int lfplus_spmv_device(lfplus_ctx *c, uint32_t j, const uint64_t *x, uint64_t n, uint64_t *y) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(spmv_impl(c, j, x, n, y, Origin::device, "lfplus_spmv_device"), oom(c, "lfplus_spmv_device: out of host memory"))
}
