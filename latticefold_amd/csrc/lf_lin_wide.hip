// lf_lin_wide.hip -- the linearization sumcheck round for the wide CCS envelope (gfx950, wave64): more than four constraint matrices (t <= 8) or a degree above
// three (d <= 7, round polynomials of degree d + 1 <= 8).  The reference's LFLinearizationProver is generic in t, q and d (sumcheck/prover.rs:56-162 with the comb
// of nifs/linearization/utils.rs:90-107); k_lin_round (lf_rounds.hip) is the kernel of its bench rows (t <= 4, d <= 3) and stays what it was.  launch_lin_round /
// launch_lin_round_fused hand every shape with desc.t > 4 or deg > 4 to launch_lin_round_wide below; nothing else comes here.
//
// Mapping: as k_lin_round -- thread = (pair, slot), slot = blockIdx.y, grid-stride over the pairs; FUSED = fix_variables of the previous round's tables inside the
// kernel, SPLIT = the per-pair eq table E_i (the host completes the message).  Differences:
//   * the table count is unrolled to 8 and the point count NP = d + 2 is a compile-time parameter (an acc[X] indexed at run time goes to scratch memory);
//   * the NP points are split over blockIdx.z in two groups of PB = ceil(NP / 2): eight tables x (value, step) x 3 words are 96 VGPRs, a lazy accumulator
//     (LH5) is 20 per point -- with all nine points resident the kernel would leave one wave per SIMD.  A block steps its tables to its first point by repeated
//     addition; with FUSED both groups fix the pair, group 0 stores it;
//   * a table is extended along X by adding its step v1 - v0 (no products); a multiset costs |S_i| - 1 products per point, one more when c_i is not +-1;
//   * the sums over a thread's pairs are lazy (LH5 column forms of AccP, lf_field.cuh) with one reduction per output at the end (generic non-residue: modular sums).
#include "lf_kernels.h"

#include "lf_kernels_dev.cuh"

namespace lf {

constexpr u32 LW_MAX_PTS = 9;                     // d + 2 <= 9
constexpr u32 LW_ROW = LW_MAX_PTS * 24;           // words per block row of `partial`: [X][3 slot + c]
constexpr u32 LW_BLOCKS = 128;                    // 128 x 216 words fit round_partial_words()

// the eight tables, written out: with the generic non-residue the compiler leaves a `#pragma unroll` loop of this size rolled, and v[j] indexed at run time
// goes to scratch memory
#define LW_EACH8(F) do { F(0); F(1); F(2); F(3); F(4); F(5); F(6); F(7); } while (0)
template <bool NU, int NP, bool FUSED, bool SPLIT>
__global__ void __launch_bounds__(256) k_lin_round_wide(DevCrt t, LinCombDesc desc, const u64 *mz, size_t ld, const u64 *eq, size_t ldeq, size_t n, u32 npts,
                                                        u64 *partial, LinFix fx, u32 xmask) {
    constexpr int PB = (NP + 1) / 2;              // points of one block
    const u32 slot = blockIdx.y, x0 = blockIdx.z * PB;
    const size_t pairs = n / 2;
    const bool store = FUSED && blockIdx.z == 0;
    LH5 acc[PB];
    Fq3 accg[PB];
#pragma unroll
    for (int i = 0; i < PB; i++) { lh5_zero(acc[i]); accg[i] = fq3_zero(); }
    const Fq3 rfix = fq3_make(fx.r.c[0], fx.r.c[1], fx.r.c[2]);
    // the fixed pair (entries 2p, 2p+1 of the new tables) of one F_{p^3} row: from the entries 4p..4p+3 of the previous one, stored when `out` is set
    auto fixed_pair = [&](const u64 *fp /* row + 4p */, size_t ldr, u64 *op /* out + 2p, or null */, size_t ldout, Fq3 &f0, Fq3 &f1) {
        const ulonglong2 a0 = *(const ulonglong2 *)(fp), a1 = *(const ulonglong2 *)(fp + ldr), a2 = *(const ulonglong2 *)(fp + 2 * ldr);
        const ulonglong2 b0 = *(const ulonglong2 *)(fp + 2), b1 = *(const ulonglong2 *)(fp + ldr + 2), b2 = *(const ulonglong2 *)(fp + 2 * ldr + 2);
        const Fq3 lo = fq3_make(a0.x, a1.x, a2.x), hi = fq3_make(b0.x, b1.x, b2.x);
        f0 = fq3_add(lo, M3<NU>(fq3_sub(fq3_make(a0.y, a1.y, a2.y), lo), rfix, t.nu));
        f1 = fq3_add(hi, M3<NU>(fq3_sub(fq3_make(b0.y, b1.y, b2.y), hi), rfix, t.nu));
        if (op) {
            *(ulonglong2 *)(op) = make_ulonglong2(f0.c[0], f1.c[0]);
            *(ulonglong2 *)(op + ldout) = make_ulonglong2(f0.c[1], f1.c[1]);
            *(ulonglong2 *)(op + 2 * ldout) = make_ulonglong2(f0.c[2], f1.c[2]);
        }
    };
    // the descriptor's per-table words, packed once into masks (bit j = table j; m_ms: four bits per table): as eight-entry arrays they stay resident in SGPRs
    // across the pair loop, and with the table pointers the kernel then spills SGPRs.  m_pos / m_neg: the multiset's coefficient is +1 / -1 (see k_lin_round)
    u32 m_live = 0, m_first = 0, m_pos = 0, m_neg = 0, m_ms = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u32 i = desc.ms[j];
        int r = desc.c_unit[0];
#pragma unroll
        for (int q = 1; q < 8; q++) r = i == (u32)q ? desc.c_unit[q] : r;
        if ((u32)j < desc.t) {
            m_live |= 1u << j;
            m_ms |= (i & 7u) << (4 * j);
            if (desc.first[j]) m_first |= 1u << j;
            if (r > 0) m_pos |= 1u << j;
            if (r < 0) m_neg |= 1u << j;
        }
    }
    const size_t tstride = 24 * ld, ostride = 24 * fx.ldo;   // table to table
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (size_t)gridDim.x * 256) {
        Fq3 v[8], st[8];
        // one per-lane pointer walks the tables (and one the fixed tables stored): eight table bases per direction would be sixteen more SGPR pairs
        const u64 *tb = mz + (size_t)3 * slot * ld + (FUSED ? 4 : 2) * p;
        u64 *ob = store ? fx.mzo + (size_t)3 * slot * fx.ldo + 2 * p : nullptr;
        // (the masks pass through an empty asm where they are tested: the compiler otherwise hoists every bit test out of the pair loop as a 64-bit lane mask,
        // some forty SGPR pairs; tested in place a bit is one s_bitcmp1_b32)
        u32 lv = m_live;
        asm volatile("" : "+s"(lv));
        auto load_table = [&](const int j) __attribute__((always_inline)) {
            if ((lv >> j) & 1) {
                if (FUSED) {
                    Fq3 f1;
                    fixed_pair(tb, ld, ob, fx.ldo, v[j], f1);
                    st[j] = fq3_sub(f1, v[j]);
                    if (store) ob += ostride;
                } else {
                    const ulonglong2 a0 = *(const ulonglong2 *)(tb), a1 = *(const ulonglong2 *)(tb + ld), a2 = *(const ulonglong2 *)(tb + 2 * ld);
                    v[j] = fq3_make(a0.x, a1.x, a2.x);
                    st[j] = fq3_sub(fq3_make(a0.y, a1.y, a2.y), v[j]);
                }
                tb += tstride;
                asm volatile("" : "+v"(tb), "+v"(ob));   // (keeps the walk in the two VGPR pairs: the compiler otherwise hoists j * stride for every j)
            } else { v[j] = fq3_zero(); st[j] = fq3_zero(); }
        };
        LW_EACH8(load_table);
        Fq3 ev, es;
        if (SPLIT) {
            es = fq3_zero();
            if (FUSED) {   // E_i[p] = E_{i-1}[2p] + E_{i-1}[2p+1]
                const ulonglong2 e0 = *(const ulonglong2 *)(eq + 2 * p), e1 = *(const ulonglong2 *)(eq + ldeq + 2 * p), e2 = *(const ulonglong2 *)(eq + 2 * ldeq + 2 * p);
                ev = fq3_make(fq_add(e0.x, e0.y), fq_add(e1.x, e1.y), fq_add(e2.x, e2.y));
                if (store && slot == 0) { fx.eqo[p] = ev.c[0]; fx.eqo[fx.ldeo + p] = ev.c[1]; fx.eqo[2 * fx.ldeo + p] = ev.c[2]; }
            } else ev = fq3_make(eq[p], eq[ldeq + p], eq[2 * ldeq + p]);
        } else if (FUSED) {
            Fq3 e1v;
            fixed_pair(eq + 4 * p, ldeq, store && slot == 0 ? fx.eqo + 2 * p : nullptr, fx.ldeo, ev, e1v);
            es = fq3_sub(e1v, ev);
        } else {
            const ulonglong2 e0 = *(const ulonglong2 *)(eq + 2 * p), e1 = *(const ulonglong2 *)(eq + ldeq + 2 * p), e2 = *(const ulonglong2 *)(eq + 2 * ldeq + 2 * p);
            ev = fq3_make(e0.x, e1.x, e2.x);
            es = fq3_sub(fq3_make(e0.y, e1.y, e2.y), ev);
        }
        // to this block's first point: x0 additions of the steps
        for (u32 k = 0; k < x0; k++) {
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = fq3_add(v[j], st[j]);
            if (!SPLIT) ev = fq3_add(ev, es);
        }
#pragma unroll 1
        for (int k = 0; k < PB; k++) {           // (rolled: its body is up to nine products; acc[] is selected by the constant-index chain below)
            const u32 X = x0 + (u32)k;
            if (X >= npts) break;
            if (!SPLIT || ((xmask >> X) & 1)) {   // (wave-uniform; SPLIT: the points not in xmask are only stepped past)
                // comb = (sum_i c_i prod_{j in S_i} v_j) * eq ; table j belongs to multiset ms[j], first[j] marks its start
                Fq3 res = fq3_zero(), term = fq3_zero();
                int sgn = 0;
                u32 kl = m_live, kf = m_first, ku = m_pos | m_neg, kn = m_neg;
                asm volatile("" : "+s"(kl), "+s"(kf), "+s"(ku), "+s"(kn));
                auto comb_table = [&](const int j) __attribute__((always_inline)) {
                    if ((kl >> j) & 1) {
                        if ((kf >> j) & 1) {      // wave-uniform
                            if (sgn) res = sgn < 0 ? fq3_sub(res, term) : fq3_add(res, term);
                            if ((ku >> j) & 1) { term = v[j]; sgn = (kn >> j) & 1 ? -1 : 1; }
                            else {
                                const u64 *cp = lin_desc_coef(desc, (m_ms >> (4 * j)) & 7u, slot);
                                term = M3<NU>(fq3_make(cp[0], cp[1], cp[2]), v[j], t.nu); sgn = 1;
                            }
                        } else term = M3<NU>(term, v[j], t.nu);
                    }
                };
                LW_EACH8(comb_table);
                if (sgn) res = sgn < 0 ? fq3_sub(res, term) : fq3_add(res, term);
                if (NU) {
                    LH5 pr;
                    lh5_zero(pr);
                    lh5_mac(pr, res, ev);
#pragma unroll
                    for (int i = 0; i < PB; i++)
                        if (k == i) {
#pragma unroll
                            for (int q = 0; q < 5; q++) { acc[i].c[q].l += pr.c[q].l; acc[i].c[q].h += pr.c[q].h; }
                        }
                } else {
                    const Fq3 gx = M3<NU>(res, ev, t.nu);
#pragma unroll
                    for (int i = 0; i < PB; i++)
                        if (k == i) accg[i] = fq3_add(accg[i], gx);
                }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = fq3_add(v[j], st[j]);
            if (!SPLIT) ev = fq3_add(ev, es);
        }
    }
    u64 vv[3 * PB];
#pragma unroll
    for (int i = 0; i < PB; i++) {
        const Fq3 r = NU ? lh5_finish(acc[i]) : accg[i];
        vv[3 * i] = r.c[0]; vv[3 * i + 1] = r.c[1]; vv[3 * i + 2] = r.c[2];
    }
    // partial[block][X][3*slot+c]: this block's points only (the other group's block writes the rest of the row)
    __shared__ u64 red[3 * PB];
    block_sum_store<3 * PB>(vv, red);
    __syncthreads();
    if (threadIdx.x < 3 * PB) {
        const u32 X = x0 + threadIdx.x / 3;
        if (X < npts) partial[(size_t)blockIdx.x * LW_ROW + X * 24 + 3 * slot + threadIdx.x % 3] = red[threadIdx.x];
    }
}

// fx != nullptr: mz / eq are the previous round's tables (2n entries per row), fixed with fx->r into fx->mzo / fx->eqo; the message is that of the fixed tables
void launch_lin_round_wide(const DevCrt &t, const LinCombDesc &desc, const u64 *mz, size_t ld, const u64 *eq, size_t ldeq, size_t n, u32 deg, u64 *partial, u64 *out,
                           hipStream_t s, u32 max_blocks, u32 xmask, const LinFix *fxp) {
    const u32 npts = deg + 1;
    if (desc.t > 8 || npts > LW_MAX_PTS) return;   // (lf_ccs_load keeps the envelope)
    u32 gb = (u32)((n / 2 + 255) / 256);
    const u32 cap = max_blocks && max_blocks < LW_BLOCKS ? max_blocks : LW_BLOCKS;
    if (gb > cap) gb = cap;
    if (gb < 1) gb = 1;
    const LinFix fx = fxp ? *fxp : LinFix{};
#define LF_LW3(NPV, F, S)                                                                                                                                   \
    do {                                                                                                                                                    \
        const dim3 grid(gb, 8, (npts + (NPV + 1) / 2 - 1) / ((NPV + 1) / 2));                                                                               \
        if (t.nu2p40) hipLaunchKernelGGL((k_lin_round_wide<true, NPV, F, S>), grid, dim3(256), 0, s, t, desc, mz, ld, eq, ldeq, n, npts, partial, fx, xmask); \
        else hipLaunchKernelGGL((k_lin_round_wide<false, NPV, F, S>), grid, dim3(256), 0, s, t, desc, mz, ld, eq, ldeq, n, npts, partial, fx, xmask);         \
    } while (0)
#define LF_LW(NPV)                                                  \
    do {                                                            \
        if (fxp) { if (xmask) LF_LW3(NPV, true, true); else LF_LW3(NPV, true, false); }    \
        else { if (xmask) LF_LW3(NPV, false, true); else LF_LW3(NPV, false, false); }      \
    } while (0)
    switch (npts) {
        case 9: LF_LW(9); break;
        case 8: LF_LW(8); break;
        case 7: LF_LW(7); break;
        case 6: LF_LW(6); break;
        default: LF_LW(5); break;   // t > 4 at d <= 3: up to five points, npts at run time
    }
#undef LF_LW
#undef LF_LW3
#undef LW_EACH8
    hipLaunchKernelGGL(k_reduce_rows, dim3(npts * 24), dim3(256), 0, s, partial, gb, LW_ROW, out);
}

}  // namespace lf
