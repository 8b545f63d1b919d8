// bb_ctx.h -- internal to the BabyBear backend's host side (bb_capi.cpp, bb_prove.cpp): the context (stream, device arena, event timeline, resident matrices
// and tables) and the helpers the two translation units share.  Not part of the C ABI.
#pragma once
#include "bb_capi.h"
#include "lf_sv_rounds.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "bb_kernels.h"
#include "lf_ajtai_i8.h"
#include "lf_common.h"
#include "lf_ctx_core.h"
#include "lf_dist.h"
#include "lf_verify.h"

namespace lfbb {

struct BbCtxImpl : CtxCore<fe> {
    BbCtxImpl() : CtxCore<fe>(16384, 5 * RE * 8 * 2) {}
    lf_ctx *owner = nullptr;
    // 0 = main work, 1 = left decomposition running concurrently (own stream, "lane1:" buffers).  A member, not the thread-local of the Goldilocks context: the
    // drivers set it and return early on errors, and they reset it at their start -- a thread-local left at 1 would leak into the next context of the thread
    int cur_lane = 0;
    int lane() const override { return cur_lane; }
    BbHostRing ring;
    DevBb dev;
    lfdist::Comm comm;               // exchange layer (lf_dist.h): RCCL communicator or host callback; the BabyBear driver exchanges from one thread only
    LinDesc desc{};
    u64 *arena[2] = {nullptr, nullptr};   // pinned staging for the asynchronous decompositions (bump-allocated per step)
    size_t arena_words = 0, arena_used[2] = {0, 0};
    hipEvent_t ev_side[2] = {nullptr, nullptr};
    hipEvent_t ev_dec[4] = {nullptr, nullptr, nullptr, nullptr};   // decomposition milestones: [2*side + (0 commit, 1 evaluations)]
    u64 *arena_alloc(size_t words) {   // nullptr when exhausted
        if (arena_used[cur_lane] + words > arena_words) return nullptr;
        u64 *r = arena[cur_lane] + arena_used[cur_lane];
        arena_used[cur_lane] += words;
        return r;
    }
};
typedef BbCtxImpl C;


// ---- shared between bb_capi.cpp / bb_prove.cpp (hidden: not part of the ABI) -----------------------------------------------------------------------
#pragma GCC visibility push(hidden)
struct BbMarks {
    bool on = false;
    std::chrono::steady_clock::time_point t0;
    double last = 0;
    void start() { on = getenv("LF_TIMELINE") != nullptr; t0 = std::chrono::steady_clock::now(); last = 0; }
    void mark(const char *what) {
        if (!on) return;
        const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[bb timeline] %-44s at %8.3f ms  (+%7.3f)\n", what, t, t - last);
        last = t;
    }
};
inline BbMarks g_marks;
#define BB_MARK(x) g_marks.mark(x)
int build_eq_dev(C *c, const H9 *pt, u32 nv, fe *eq_dev);
int down_small(C *c, const u64 *dsrc, size_t words, u64 *host);
int exchange_modsum(C *c, u64 *inout, size_t words);
int build_eq_async(C *c, const H9 *pt, u32 nv, fe *eq_dev);
int build_z(C *c, const int32_t *planes, u32 K, int mode_bits, const u64 *heads, fe *z);   // bb_prove.cpp (synchronises the stream)
#pragma GCC visibility pop

}  // namespace lfbb
