// lf_check.hip -- gfx950 kernels of the relation checks (lf_check.cpp): the CCS residual of CCS::check_relation (arith.rs:76-110) on the Goldilocks ring, and
// the l-infinity norm of a witness straight from its int32 coefficient planes (both rings).  The BabyBear residual is bb_check.hip.
//
// Residual: one thread per (row, slot), slot = blockIdx.y, so that a wave reads 64 consecutive rows of every plane (coalesced 8-byte loads).  The comb is
// k_lin_round's (lf_rounds.hip): tables of one multiset are consecutive, `first[j]` starts a multiset, c_unit skips the product by +-1.  A wave that sees a
// non-zero residual takes the lowest such lane -- rows grow with the lane, so that is the wave's smallest bad row -- and that lane alone issues one global
// atomic min.  A satisfied system issues none.
#include "lf_check.h"

#include "lf_kernels_dev.cuh"

namespace lf {

template <bool NU, int TT>   // TT = 4: the bench envelope (t <= 4); 8: the wide envelope
__global__ void __launch_bounds__(256) k_ccs_residual(DevCrt t, LinCombDesc desc, const u64 *mz, size_t ld, size_t m, u32 *first_bad) {
    const u32 slot = blockIdx.y;
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    // the unit coefficients of the tables' multisets, selected once (see k_lin_round: a dynamically indexed field of the by-value descriptor would be
    // copied to scratch memory)
    int cu_j[TT];
#pragma unroll
    for (int j = 0; j < TT; j++) {
        const u32 i = desc.ms[j];
        int r = desc.c_unit[0];
#pragma unroll
        for (int q = 1; q < 8; q++) r = i == (u32)q ? desc.c_unit[q] : r;
        cu_j[j] = r;
    }
    bool bad = false;
    if (row < m) {
        Fq3 res = fq3_zero(), term = fq3_zero();
        int sgn = 0;
#pragma unroll
        for (int j = 0; j < TT; j++) {
            if ((u32)j < desc.t) {
                const Fq3 v = ld3(mz + (size_t)j * 24 * ld, ld, slot, row);
                if (desc.first[j]) {   // (wave-uniform)
                    if (sgn) res = sgn < 0 ? fq3_sub(res, term) : fq3_add(res, term);
                    if (cu_j[j]) { term = v; sgn = cu_j[j]; }
                    else {
                        const u32 i = desc.ms[j];
                        if (TT > 4) {   // (from the kernel-argument segment: eight tables leave no room for a scratch copy of the descriptor)
                            const u64 *cp = lin_desc_coef(desc, i, slot);
                            term = M3<NU>(fq3_make(cp[0], cp[1], cp[2]), v, t.nu);
                        } else
                        term = M3<NU>(fq3_make(desc.c[i][3 * slot], desc.c[i][3 * slot + 1], desc.c[i][3 * slot + 2]), v, t.nu);
                        sgn = 1;
                    }
                } else term = M3<NU>(term, v, t.nu);
            }
        }
        if (sgn) res = sgn < 0 ? fq3_sub(res, term) : fq3_add(res, term);
        bad = (res.c[0] | res.c[1] | res.c[2]) != 0;   // canonical residues: zero is the word 0
    }
    const unsigned long long mask = __ballot(bad);
    if (mask && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mask) - 1)) atomicMin(first_bad, (u32)row);
}
void launch_ccs_residual(const DevCrt &t, const LinCombDesc &desc, const u64 *mz, size_t ld, size_t m, u32 *first_bad, hipStream_t s) {
    if (!m) return;
    const dim3 grid(cdiv(m, 256), 8);
    if (desc.t > 4) {
        if (t.nu2p40) hipLaunchKernelGGL((k_ccs_residual<true, 8>), grid, dim3(256), 0, s, t, desc, mz, ld, m, first_bad);
        else hipLaunchKernelGGL((k_ccs_residual<false, 8>), grid, dim3(256), 0, s, t, desc, mz, ld, m, first_bad);
        return;
    }
    if (t.nu2p40) hipLaunchKernelGGL((k_ccs_residual<true, 4>), grid, dim3(256), 0, s, t, desc, mz, ld, m, first_bad);
    else hipLaunchKernelGGL((k_ccs_residual<false, 4>), grid, dim3(256), 0, s, t, desc, mz, ld, m, first_bad);
}

// max |v| over the int32 planes: a grid-stride pass, a wave maximum by shuffles, one atomic max per wave with a non-zero maximum
__global__ void __launch_bounds__(256) k_planes_absmax(const int32_t *planes, size_t count, u32 *out) {
    u32 mx = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const int32_t v = planes[i];
        const u32 a = v < 0 ? 0u - (u32)v : (u32)v;   // (|INT32_MIN| = 2^31 fits)
        mx = a > mx ? a : mx;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u32 o = (u32)__shfl_xor((int)mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(out, mx);
}
void launch_planes_absmax(const int32_t *planes, size_t count, u32 *out, hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL(k_planes_absmax, dim3(grid_for(count, 1024)), dim3(256), 0, s, planes, count, out);
}

}  // namespace lf
