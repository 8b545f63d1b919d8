// bb_check.hip -- BabyBear backend: the CCS residual of CCS::check_relation (arith.rs:76-110) in F_{p^9} slots (bb_check.cpp).  Same shape as
// lf_check.hip's k_ccs_residual: one thread per (row, slot), the comb of bb_rounds.hip's k_lin_round, the wave's lowest bad lane issues the one atomic min.
#include "lf_check.h"

#include "bb_kernels_dev.cuh"

namespace lfbb {

__device__ __forceinline__ E9 pick_t(const E9 (&v)[4], u32 idx) {
    E9 r;
#pragma unroll
    for (int c = 0; c < TAU; c++) r.c[c] = idx == 0 ? v[0].c[c] : (idx == 1 ? v[1].c[c] : (idx == 2 ? v[2].c[c] : v[3].c[c]));
    return r;
}

__global__ void __launch_bounds__(256) k_ccs_residual(DevBb t, LinDesc desc, const fe *mz, size_t ld, size_t m, u32 *first_bad) {
    const u32 slot = blockIdx.y;
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (row < m) {
        E9 v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = (u32)j < desc.t ? ld9(mz + (size_t)j * RE * ld, ld, slot, row) : e9_zero();
        E9 sum = e9_zero();
        for (u32 i = 0; i < desc.q; i++) {
            const u32 k0 = desc.S_off[i], k1 = desc.S_off[i + 1];
            E9 term = pick_t(v, desc.S_idx[k0]);
            for (u32 k = k0 + 1; k < k1; k++) term = e9_mul(term, pick_t(v, desc.S_idx[k]), t.nu);
            if (desc.c_unit[i] == 1) sum = e9_add(sum, term);
            else if (desc.c_unit[i] == -1) sum = e9_sub(sum, term);
            else {
                E9 cc;
#pragma unroll
                for (int c = 0; c < TAU; c++) cc.c[c] = desc.c[i][TAU * slot + c];
                sum = e9_add(sum, e9_mul(term, cc, t.nu));
            }
        }
        fe any = 0;
#pragma unroll
        for (int c = 0; c < TAU; c++) any |= sum.c[c];   // centred words in [-H, H]: zero is the word 0
        bad = any != 0;
    }
    const unsigned long long mask = __ballot(bad);
    if (mask && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mask) - 1)) atomicMin(first_bad, (u32)row);
}
void launch_ccs_residual(const DevBb &t, const LinDesc &desc, const fe *mz, size_t ld, size_t m, u32 *first_bad, hipStream_t s) {
    if (!m) return;
    hipLaunchKernelGGL(k_ccs_residual, dim3(cdiv(m, 256), 8), dim3(256), 0, s, t, desc, mz, ld, m, first_bad);
}

}  // namespace lfbb
