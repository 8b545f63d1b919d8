// lfp_tables.cpp -- host bodies of the "MLE tables on arrays" section of include/lfplus.h: lfplus_build_eq, lfplus_mle_eval_batch, lfplus_mle_fix_variables,
// lfplus_spmv_t and their _device forms (kernels: lfp_tables.hip).  One body per call for both memory spaces: a host array is staged through the context's
// pooled scratch, a device array is read and written in place.  Points and the results of lfplus_mle_eval_batch are small and stay on the host.
//   Nothing resident is read or written: the buffers are the call's own blocks of the pool (given back before it returns), the work runs on the context's first
// stream, and neither the witness, the from_f results, a pass pending on the second stream nor the state of a generic sumcheck is looked at.  lfplus_spmv_t reads
// the transposed structure the resident matrices carry since their upload (LfpMatrix colptr / rowidx / valT: owned by the reference-counted MatsOwner, so a
// context that shares the matrices shares it, and it goes when they are replaced).
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
    const char *e = getenv("LFPLUS_TABLE_BLOCKS");   // workgroups of lfplus_build_eq / lfplus_mle_eval_batch at most (default 2048: 8 per CU); read once per call
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= 65535 ? (u32)v : 2048u;
}
lfp::TabPoint point_mont(const u64 *r, u32 first, u32 count) {
    lfp::TabPoint pt;
    memset(&pt, 0, sizeof(pt));
    for (u32 i = 0; i < count; i++) pt.rM[i] = to_mont(r[first + i]);
    pt.oneM = to_mont(1);
    return pt;
}
// the word flag comes home (with `extra` bytes of a small device result, if any) and the stream is drained
hipError_t fetch_flag(lfplus_ctx *c, const u32 *dflag, u32 *flag, void *dst = nullptr, const void *src = nullptr, size_t extra = 0) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(flag, dflag, 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess && extra) e = hipMemcpyAsync(dst, src, extra, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    return e;
}

int build_eq_impl(lfplus_ctx *c, const uint64_t *point, uint32_t nv, uint64_t *out, Origin o, const char *who) {
    const std::string w(who);
    if (!point || !out) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (nv < 1 || nv > 28) return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= nv <= 28)");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const bool dev = o == Origin::device;
    const u64 entries = 1ull << nv, obytes = entries * 128;
    if (!dev && ranges_overlap(out, obytes, point, (u64)nv * 8)) return fail(c, LFPLUS_E_ARG, w + ": out overlaps the point");
    if (dev && lfp_dev_ptr_check(c, out, entries, who)) return LFPLUS_E_ARG;
    if (!canonical(point, nv)) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in point");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    u64 *dout = out;
    if (!dev && !sc.get(&dout, obytes)) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    lfp::launch_tab_eq(point_mont(point, 0, nv), nv, dout, block_cap(), c->st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !dev) e = hipMemcpyAsync(out, dout, obytes, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return hip_fail(c, w, e);
    return LFPLUS_OK;
}

int eval_impl(lfplus_ctx *c, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point, uint32_t nv, uint64_t *out, Origin o, const char *who) {
    const std::string w(who);
    if (!tables || !point || !out) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (ntables < 1 || ntables > 64 || nv < 1 || nv > 28 || len < 1 || len > (1ull << nv))
        return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= ntables <= 64, 1 <= nv <= 28, 1 <= len <= 2^nv)");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const bool dev = o == Origin::device;
    const u64 tbytes = (u64)ntables * len * 128, obytes = (u64)ntables * 128;
    // (out and the point are host memory in both spellings; device tables share no address space with them)
    if (ranges_overlap(out, obytes, point, (u64)nv * 8) || (!dev && ranges_overlap(out, obytes, tables, tbytes)))
        return fail(c, LFPLUS_E_ARG, w + ": out overlaps an input");
    if (dev && lfp_dev_ptr_check(c, tables, (u64)ntables * len, who)) return LFPLUS_E_ARG;
    if (!canonical(point, nv)) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in point");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const u32 blocks = lfp::tab_eval_blocks(len, nv, ntables, block_cap());
    const u64 *dt = tables;
    u64 *tt = nullptr, *part = nullptr, *res = nullptr;
    u32 *dflag = nullptr;
    bool ok = sc.get(&dflag, 8) && sc.get(&part, (size_t)ntables * blocks * 128) && sc.get(&res, obytes);
    if (ok && !dev) ok = sc.get(&tt, tbytes);
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    hipError_t e = hipMemsetAsync(dflag, 0, 4, c->st);
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(tt, tables, tbytes, hipMemcpyHostToDevice, c->st);
        dt = tt;
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    lfp::launch_tab_eval(dt, ntables, len, point_mont(point, 0, nv), nv, blocks, part, res, dflag, c->st);
    u32 flag = 0;
    std::vector<u64> hres((size_t)ntables * 16);
    e = fetch_flag(c, dflag, &flag, hres.data(), res, obytes);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (flag) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in tables");
    memcpy(out, hres.data(), obytes);
    return LFPLUS_OK;
}

int fix_impl(lfplus_ctx *c, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point, uint32_t nfix, uint64_t *out, Origin o, const char *who) {
    const std::string w(who);
    if (!tables || !point || !out) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    u32 nv = 0;
    while (nv < 28 && (1ull << nv) < len) nv++;
    if (ntables < 1 || ntables > 64 || len < 2 || len != (1ull << nv) || nfix < 1 || nfix > nv)
        return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= ntables <= 64, len = 2^nv with 1 <= nv <= 28, 1 <= nfix <= nv)");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const bool dev = o == Origin::device;
    const u64 nout = len >> nfix, tbytes = (u64)ntables * len * 128, obytes = (u64)ntables * nout * 128;
    if (ranges_overlap(out, obytes, tables, tbytes) || (!dev && ranges_overlap(out, obytes, point, (u64)nfix * 8)))
        return fail(c, LFPLUS_E_ARG, w + ": out overlaps an input");
    if (dev && (lfp_dev_ptr_check(c, tables, (u64)ntables * len, who) || lfp_dev_ptr_check(c, out, (u64)ntables * nout, who))) return LFPLUS_E_ARG;
    if (!canonical(point, nfix)) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in point");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    // more than TAB_FIX variables: a chain of launches through two scratch tables (the first reads the caller's tables once and leaves a 64th of them)
    const u32 steps = (nfix + lfp::TAB_FIX - 1) / lfp::TAB_FIX;
    const u64 *dt = tables;
    u64 *tt = nullptr, *dout = out, *mid[2] = {nullptr, nullptr};
    u32 *dflag = nullptr;
    bool ok = sc.get(&dflag, 8);
    if (ok && !dev) ok = sc.get(&tt, tbytes) && sc.get(&dout, obytes);
    if (ok && steps > 1) ok = sc.get(&mid[0], (size_t)ntables * (len >> lfp::TAB_FIX) * 128);
    if (ok && steps > 2) ok = sc.get(&mid[1], (size_t)ntables * (len >> (2 * lfp::TAB_FIX)) * 128);
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    hipError_t e = hipMemsetAsync(dflag, 0, 4, c->st);
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(tt, tables, tbytes, hipMemcpyHostToDevice, c->st);
        dt = tt;
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    const u64 *src = dt;
    u64 cur = len;
    for (u32 s = 0, done = 0; s < steps; s++) {
        const u32 nf = nfix - done < lfp::TAB_FIX ? nfix - done : lfp::TAB_FIX;
        u64 *dst = s + 1 == steps ? dout : mid[s & 1];
        lfp::launch_tab_fix(src, cur, ntables, cur >> nf, point_mont(point, done, nf), nf, dst, dflag, c->st);
        src = dst;
        cur >>= nf;
        done += nf;
    }
    u32 flag = 0;
    e = fetch_flag(c, dflag, &flag);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (flag) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in tables");
    if (!dev) {
        e = hipMemcpyAsync(out, dout, obytes, hipMemcpyDeviceToHost, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) return hip_fail(c, w, e);
    }
    return LFPLUS_OK;
}

int spmv_t_impl(lfplus_ctx *c, uint32_t j, const uint64_t *v, uint64_t n, uint64_t *out, Origin o, const char *who) {
    const std::string w(who);
    if (!v || !out) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (c->mats.empty()) return fail(c, LFPLUS_E_ARG, w + ": no resident matrices (lfplus_set_matrices / lfplus_share_matrices)");
    if (j >= c->mats.size()) return fail(c, LFPLUS_E_ARG, w + ": matrix " + std::to_string(j) + " of " + std::to_string(c->mats.size()));
    if (n != c->mats_n) return fail(c, LFPLUS_E_ARG, w + ": n = " + std::to_string(n) + ", the resident matrices are " + std::to_string(c->mats_n) + " wide");
    if (c->sharded()) return fail(c, LFPLUS_E_ARG, w + ": sharded contexts are not supported");
    const u64 bytes = n * 128;
    if (ranges_overlap(v, bytes, out, bytes)) return fail(c, LFPLUS_E_ARG, w + ": out overlaps v (the product gathers)");
    const bool dev = o == Origin::device;
    if (dev && (lfp_dev_ptr_check(c, v, n, who) || lfp_dev_ptr_check(c, out, n, who))) return LFPLUS_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const u64 *dv = v;
    u64 *dout = out, *tv = nullptr;
    u32 *dflag = nullptr;
    bool ok = sc.get(&dflag, 8);
    if (ok && !dev) ok = sc.get(&tv, bytes) && sc.get(&dout, bytes);
    if (!ok) return fail(c, LFPLUS_E_HIP, w + ": out of device memory");
    hipError_t e = hipMemsetAsync(dflag, 0, 4, c->st);
    if (e == hipSuccess && !dev) {
        e = hipMemcpyAsync(tv, v, bytes, hipMemcpyHostToDevice, c->st);
        dv = tv;
    }
    if (e != hipSuccess) return hip_fail(c, w, e);
    const LfpMatrix &m = c->mats[j];
    lfp::launch_check_canonical(dv, (size_t)n * 16, dflag, 1u, c->st);
    lfp::launch_spmv_t(m.colptr, m.rowidx, m.valT, dv, n, dout, c->st);      // (row indices and the column pointers were built from the validated CSR at the upload)
    u32 flag = 0;
    e = fetch_flag(c, dflag, &flag);
    if (e != hipSuccess) return hip_fail(c, w, e);
    if (flag) return fail(c, LFPLUS_E_ARG, w + ": non-canonical word in v");
    if (!dev) {
        e = hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) return hip_fail(c, w, e);
    }
    return LFPLUS_OK;
}
}  // namespace

// a NULL context is LFPLUS_E_ARG before any device is touched: the answer on a machine without a GPU as well
extern "C" int lfplus_build_eq(lfplus_ctx *c, const uint64_t *point, uint32_t nv, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(build_eq_impl(c, point, nv, out, Origin::host, "lfplus_build_eq"), oom(c, "lfplus_build_eq: out of host memory"))
}
extern "C" int lfplus_build_eq_device(lfplus_ctx *c, const uint64_t *point, uint32_t nv, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(build_eq_impl(c, point, nv, out, Origin::device, "lfplus_build_eq_device"), oom(c, "lfplus_build_eq_device: out of host memory"))
}
extern "C" int lfplus_mle_eval_batch(lfplus_ctx *c, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point, uint32_t nv, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(eval_impl(c, tables, ntables, len, point, nv, out, Origin::host, "lfplus_mle_eval_batch"), oom(c, "lfplus_mle_eval_batch: out of host memory"))
}
extern "C" int lfplus_mle_eval_batch_device(lfplus_ctx *c, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point, uint32_t nv, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(eval_impl(c, tables, ntables, len, point, nv, out, Origin::device, "lfplus_mle_eval_batch_device"), oom(c, "lfplus_mle_eval_batch_device: out of host memory"))
}
extern "C" int lfplus_mle_fix_variables(lfplus_ctx *c, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point, uint32_t nfix, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(fix_impl(c, tables, ntables, len, point, nfix, out, Origin::host, "lfplus_mle_fix_variables"), oom(c, "lfplus_mle_fix_variables: out of host memory"))
}
extern "C" int lfplus_mle_fix_variables_device(lfplus_ctx *c, const uint64_t *tables, uint32_t ntables, uint64_t len, const uint64_t *point, uint32_t nfix, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(fix_impl(c, tables, ntables, len, point, nfix, out, Origin::device, "lfplus_mle_fix_variables_device"),
              oom(c, "lfplus_mle_fix_variables_device: out of host memory"))
}
extern "C" int lfplus_spmv_t(lfplus_ctx *c, uint32_t j, const uint64_t *v, uint64_t n, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(spmv_t_impl(c, j, v, n, out, Origin::host, "lfplus_spmv_t"), oom(c, "lfplus_spmv_t: out of host memory"))
}
extern "C" int lfplus_spmv_t_device(lfplus_ctx *c, uint32_t j, const uint64_t *v, uint64_t n, uint64_t *out) {
    if (!c) return LFPLUS_E_ARG;
    LFP_GUARD(spmv_t_impl(c, j, v, n, out, Origin::device, "lfplus_spmv_t_device"), oom(c, "lfplus_spmv_t_device: out of host memory"))
}
