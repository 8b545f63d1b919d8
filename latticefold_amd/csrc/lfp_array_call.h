// lfp_array_call.h -- what the host bodies of the calls on caller-owned arrays share (lfp_ring_ops.cpp: lfplus_ring_mul / lfplus_spmv; lfp_tables.cpp: lfplus_build_eq,
// lfplus_mle_eval_batch, lfplus_mle_fix_variables, lfplus_spmv_t; lfp_digits.cpp: lfplus_balanced_decompose / _recompose, lfplus_linf_norm): the overlap test, the call's scratch, the way out after a failure inside the enqueued part
#pragma once
#include <string>
#include <vector>
#include "lfp_ctx.h"

namespace lfp_arr {
inline u64 to_mont(u64 a) { return (u64)((((unsigned __int128)a) << 64) % lfp::P); }
inline bool ranges_overlap(const void *a, u64 abytes, const void *b, u64 bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bbytes && pb < pa + abytes;
}
// the call's own scratch: blocks of the context's pool (which releases the process-wide cache and retries before it gives up), given back on every way out
struct Scratch {
    lfplus_ctx *c;
    std::vector<void *> held;
    explicit Scratch(lfplus_ctx *ctx) : c(ctx) {}
    ~Scratch() { for (void *p : held) c->own_free(p); }
    template <class T> bool get(T **p, size_t bytes) {
        if (c->own_alloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        held.push_back((void *)*p);
        return true;
    }
};
// after a failure inside the enqueued part: the stream is drained before the scratch goes back to the pool
inline int hip_fail(lfplus_ctx *c, const std::string &who, hipError_t e) {
    (void)hipStreamSynchronize(c->st);
    (void)hipGetLastError();
    return fail(c, LFPLUS_E_HIP, who + ": " + hipGetErrorString(e));
}
inline int oom(lfplus_ctx *c, const char *m) {
    try { c->err = m; } catch (...) {}
    return LFPLUS_E_HIP;
}
}  // namespace lfp_arr
