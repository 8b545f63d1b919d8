// lf_check.h -- launchers of the relation-check kernels (lf_check.hip, bb_check.hip): the CCS residual with its first-bad-row reduction, and the
// largest |coefficient| of a witness's int32 planes.  All pointers are DEVICE pointers.
#pragma once
#include "bb_kernels.h"
#include "lf_kernels.h"

namespace lf {
// CCS::check_relation (arith.rs:76-110) on materialised tables mz [t][24][ld] = M_j z: for every row < m the residual sum_i c_i (.) prod_{j in S_i} mz_j[row],
// slot by slot.  *first_bad (u32, set to m by the caller) is lowered to the smallest row with a non-zero residual (one atomic min per wave that saw one).
void launch_ccs_residual(const DevCrt &t, const LinCombDesc &desc, const u64 *mz, size_t ld, size_t m, u32 *first_bad, hipStream_t s);
// *out (u32, zeroed by the caller) is raised to max |planes[i]| over `count` int32 words (both rings: the planes hold centred integers)
void launch_planes_absmax(const int32_t *planes, size_t count, u32 *out, hipStream_t s);
}  // namespace lf

namespace lfbb {
// the BabyBear twin of lf::launch_ccs_residual: mz [t][72][ld] centred Montgomery words, F_{p^9} slots
void launch_ccs_residual(const DevBb &t, const LinDesc &desc, const fe *mz, size_t ld, size_t m, u32 *first_bad, hipStream_t s);
}  // namespace lfbb
