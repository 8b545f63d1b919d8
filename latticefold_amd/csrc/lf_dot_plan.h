// lf_dot_plan.h -- the ONE test "the int8 form of the inner products takes this shape" of the Goldilocks path, on top of the host's plan of a call (DotPlan,
// lf_dot_i8.cuh).  Host code only: the drivers evaluate the test before they enqueue the q_j gathers, the launchers evaluate the same test, and the stand-alone
// lf_q_pack_selftest.cpp includes this file without a device compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lf_dot_i8.cuh"

namespace lf {
constexpr uint32_t DOT_CHUNKS = 40;   // 24 units x 40 chunks = 240 blocks of 4 waves: ONE batch on 256 CUs at one wave per SIMD (44 chunks = 264 blocks ran as two batches: 2x the time)
// One launch of k_dot_i8 takes this shape: na <= 16 vectors X [24][ldx] (rows on two-word boundaries: even ldx) against nb <= 3 vectors Y over n >= 64
// columns, the words aligned and a wave's int32 accumulators exact (DotPlan::make).  launch_dot_batch_i8 / launch_dot_pack_y / launch_q_pack_i8 decline
// (I8_ERR_SHAPE) exactly where this is false.
inline bool dot_i8_shape(const uint64_t *X, size_t ldx, uint32_t na, uint32_t nb, size_t n, i8mma::DotPlan *p) {
    return na >= 1 && na <= 16 && nb >= 1 && nb <= 3 && !(ldx & 1) && p->make(X, n, DOT_CHUNKS);
}
// ... and the drivers send it there: the shape above, from dot_min columns on, unless LF_DOT_VALU asks for the 64-bit kernel.  Evaluated BEFORE the q_j
// gathers are enqueued: where it holds (and the slice needs no lead column) they write the packed digits and no words (k_q_pack_i8).
inline bool dot_i8_takes(bool dot_valu, size_t dot_min, const uint64_t *X, size_t ldx, uint32_t na, uint32_t nb, size_t n, i8mma::DotPlan *p) {
    return !dot_valu && n >= dot_min && dot_i8_shape(X, ldx, na, nb, n, p);
}
}  // namespace lf
