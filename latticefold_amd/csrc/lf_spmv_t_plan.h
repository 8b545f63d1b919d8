// lf_spmv_t_plan.h -- host side of lf_spmv_t's heavy-column path (lf_spmv_t.cuh): the two constants of the split and the work list lf_ccs_load builds from the
// column pointers of a matrix.  Host only; the kernels' header includes it for the constants.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace lfk {

// A column with at least SPMV_T_HEAVY entries leaves the light path (one thread per (column, slot)) for the heavy one (one block per work item).  Measured
// on the MI355X (raw output profiles/witness_tables_measure.txt): 512 columns of c entries each, every column heavy against none -- 0.106 /
// 0.113 ms at c = 16, 0.128 / 0.131 at 32, 0.137 / 0.161 at 64, 0.119 / 0.201 at 128, 0.142 / 0.261 at 256, 0.148 / 0.848 at 1024: level up to 32 entries,
// the heavy path ahead from 64 on.  The constant column of a 2^20-row matrix: 0.377 ms with the heavy path, 794 ms as one thread's walk.
constexpr uint32_t SPMV_T_HEAVY = 64;
// ... and is cut into work items of at most SPMV_T_CHUNK consecutive entries of its CSC range: 32 entries side by side, 16 trips per thread.  512 is not the
// result of a sweep: it is the largest power of two that lets a 1024-row test matrix span several items, and at 2^20 entries it gives 2048 blocks (eight per
// CU) and 2048 partial elements for the column's sum kernel -- 0.377 ms for 201 MB of matrix values, the time of the one-entry-per-row matrices of that size
constexpr uint32_t SPMV_T_CHUNK = 512;

// plan = nitems triples (column, k0, k1), k1 - k0 <= SPMV_T_CHUNK, then ncols triples (column, first item, one past its last item); empty without heavy columns
static inline void spmv_t_plan(size_t n, const uint32_t *colptr, uint32_t heavy_min, std::vector<uint32_t> *plan, uint32_t *nitems, uint32_t *ncols) {
    std::vector<uint32_t> items, cols;
    for (size_t c = 0; c < n; c++) {
        const uint32_t k0 = colptr[c], k1 = colptr[c + 1];
        if (k1 - k0 < heavy_min || k1 == k0) continue;
        const uint32_t first = (uint32_t)(items.size() / 3);
        for (uint32_t k = k0; k < k1; k += SPMV_T_CHUNK) {
            items.push_back((uint32_t)c); items.push_back(k); items.push_back(k1 - k < SPMV_T_CHUNK ? k1 : k + SPMV_T_CHUNK);
        }
        cols.push_back((uint32_t)c); cols.push_back(first); cols.push_back((uint32_t)(items.size() / 3));
    }
    *nitems = (uint32_t)(items.size() / 3);
    *ncols = (uint32_t)(cols.size() / 3);
    plan->swap(items);
    plan->insert(plan->end(), cols.begin(), cols.end());
}

}  // namespace lfk
