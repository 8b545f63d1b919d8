// lf_dot_i8.hip -- batched inner products of F_{p^3}-slot vectors on the int8 matrix cores (gfx950 v_mfma_i32_16x16x64_i8):
//     out[a][b][slot] = sum_i X_a[slot][i] * Y_b[slot][i]        (a < na <= 16 vectors X, b < nb <= 3 vectors Y, 8 slots, n columns)
// -- the u_s and eta evaluations of a fold step (decomposition.rs:214-256, folding.rs:236-256: <z_k, M_j^T eq(r)>), was k_dot_batch:
// 48 lazy 64-bit F_{p^3} multiply-accumulates per column and slot on the quarter-rate integer multiplier, 0.48 ms per call at C4.
//
// Every 64-bit word of both operands is written with balanced base-256 digits (d_u in [-128, 127], sum_u d_u 256^u = the word or the word - p:
// byte_u(w + 0x80..80) ^ 0x80, see lf_sv_rounds.hip), so a product of two words is sum_{u,v} 256^(u+v) d_u e_v and the sums over the columns
// of all digit products are an exact int8 GEMM: per (slot, component cz of X) rows = (digit u, vector a) -- 8 row tiles of 16 vectors --,
// inner dimension = columns, matrix columns = (vector b, component cq, digit v) of Y -- 72 = 5 column tiles.  The X digits are cut in
// registers from the 16 words a lane loads (every byte of every word is used once: X streams from HBM exactly once); the Y digits are packed
// once per call (k_dot_pack_y: Y is 1/5 of X).  F_{p^3} structure, powers of 256 and the reduction mod p happen once per output.
#include <hip/hip_runtime.h>
#include "lf_field.cuh"
#include "lf_kernels.h"
#include "lf_dot_i8.cuh"
#include "lf_dot_plan.h"

namespace lf {
using namespace i8mma;

struct DotI8Args : DotArgs<u64> {};   // X [na][24][ldx], YB [8][72][ldq], part [unit 24][chunk][u 8][nt 5][64][4]

// one K-step: digits of the 16 words, the 8 digit-plane operands (register j of digit u = bytes u of words 4j .. 4j+3), 40 MFMAs
__device__ __forceinline__ void dot_step(v4i (&acc)[8][5], const u64 (&raw)[16], const v4i (&b)[5]) {
    u64 w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) w[t] = balanced_bytes(raw[t]);
#pragma unroll
    for (int u = 0; u < 8; u++) {
        u32 op[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32 h0 = u < 4 ? (u32)w[4 * j] : (u32)(w[4 * j] >> 32), h1 = u < 4 ? (u32)w[4 * j + 1] : (u32)(w[4 * j + 1] >> 32);   // the half that holds digit u
            const u32 h2 = u < 4 ? (u32)w[4 * j + 2] : (u32)(w[4 * j + 2] >> 32), h3 = u < 4 ? (u32)w[4 * j + 3] : (u32)(w[4 * j + 3] >> 32);
            op[j] = gather_bytes(h0, h1, h2, h3, u & 3);
        }
        const v4i av = v4i{(int)op[0], (int)op[1], (int)op[2], (int)op[3]};
#pragma unroll
        for (int nt = 0; nt < 5; nt++) acc[u][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b[nt], acc[u][nt], 0, 0, 0);
    }
}
// wave = one (slot, cz) unit x one chunk of columns.  One wave per SIMD (160 accumulator registers): the loads of the next K-step are in
// flight while this one is computed (two K-steps ahead needed more registers than the file has next to the accumulators).
// This kernel rotates three operand buffers, lfbb::k_bbdot_i8 (bb_dot_i8.hip) two: the two software pipelines were tuned separately, each against its own
// accumulator count (160 / 112 registers), and both stay -- only the helpers of lf_i8_mma.cuh are shared.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_dot_i8(DotI8Args a) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, g = lane >> 4;
    // 1-D grid of 24 * nq blocks (nq = chunk quads).  Workgroups go round-robin to the 8 XCDs, and the three cz units of a (slot, chunk quad)
    // read the same Y digits: block L = x + 8 cz + 24 j handles combo x + 8 j, so the three land on one XCD, 8 apart in dispatch order,
    // and share those digits in its L2 (PMC: 1275 -> 1005 MB fetched per launch for 805 + 151 MB of operands; the duration did not move)
    const u32 L = blockIdx.x, combo = (L % 8) + 8 * (L / 24), cz = (L / 8) % 3;
    const u32 slot = combo % 8, unit = slot * 3 + cz;
    const u32 chunk = (combo / 8) * 4 + wave;
    v4i acc[8][5];
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
        for (int nt = 0; nt < 5; nt++) acc[u][nt] = v4i{0, 0, 0, 0};
    if (chunk >= a.chunks) return;
    const u32 s0 = chunk * a.steps_per_chunk, s1 = s0 + a.steps_per_chunk < a.nsteps ? s0 + a.steps_per_chunk : a.nsteps;
    const u64 *xrow = a.X + ((size_t)row * 24 + 3 * slot + cz) * a.ldx;
    const bool xlive = row < a.na;
    const unsigned char *yb = a.YB + (size_t)slot * 72 * a.ldq;
    const u32 last = s1 > s0 ? s1 - 1 : s0;
    auto colw = [&](u32 st) { return (size_t)(st < last ? st : last) * 64; };   // clamped: the tail re-loads the last step
    // TWO K-steps in flight (the accumulators live in AGPRs, so 256 - 153 vector registers were idle: one step ahead left a wave -- the only one of its SIMD --
    // with 8 KB outstanding, and the kernel at 2.5 TB/s)
    u64 xa[16], xn[16], xm[16];
    v4i ba[5], bn[5], bm[5];
    dot_load_x(xrow, colw(s0), g, a.n, xlive, xa); dot_load_y(yb, a.ldq, colw(s0) + 16 * g, row, a.nrows_y, ba);
    dot_load_x(xrow, colw(s0 + 1), g, a.n, xlive && s0 + 1 < s1, xn); dot_load_y(yb, a.ldq, colw(s0 + 1) + 16 * g, row, a.nrows_y, bn);
    // (three buffers in rotation, the loop unrolled by three: a register copy of a buffer would wait for its load at the end of the very step that issued it.  No
    // exits inside the trip -- control flow around the MFMA block makes the compiler copy the tied accumulators: 359 spilled registers --: the last trip is padded
    // with steps whose X words are zero)
    auto ldx = [&](u32 st, u64 (&dst)[16]) { dot_load_x(xrow, colw(st), g, a.n, xlive && st < s1, dst); };
    for (u32 st = s0; st < s1; st += 3) {
        ldx(st + 2, xm); dot_load_y(yb, a.ldq, colw(st + 2) + 16 * g, row, a.nrows_y, bm);   // two K-steps ahead
        dot_step(acc, xa, ba);
        ldx(st + 3, xa); dot_load_y(yb, a.ldq, colw(st + 3) + 16 * g, row, a.nrows_y, ba);
        dot_step(acc, xn, bn);
        ldx(st + 4, xn); dot_load_y(yb, a.ldq, colw(st + 4) + 16 * g, row, a.nrows_y, bn);
        dot_step(acc, xm, bm);
    }
    int32_t *o = a.part + ((size_t)unit * a.chunks + chunk) * (8 * 5 * 256);
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
        for (int nt = 0; nt < 5; nt++) *(v4i *)(o + ((size_t)u * 5 + nt) * 256 + lane * 4) = acc[u][nt];
}

// block = output (a, b, slot, comp), thread = (cz, digit u):  out[(a*nb + b)*24 + 3*slot + comp] = sum over (cz, cq) with cz + cq = comp (mod 3) of
// nu^[cz+cq >= 3] * sum_{u,v} 256^(u+v) tot[slot, cz][u][a][(b, cq, v)]
__global__ void __launch_bounds__(32) k_dot_i8_finish(const long long *tot, u32 na, u32 nb, u64 nu, u64 *out, u32 nb_out, u32 b0) {
    __shared__ u64 sm[24];
    const u32 o = blockIdx.x, t = threadIdx.x;
    const u32 comp = o % 3, slot = (o % 24) / 3, b = (o / 24) % nb, av = o / (24 * nb);
    if (t < 24) {
        const u32 cz = t >> 3, u = t & 7, cq = (comp + 3 - cz) % 3;
        const long long *tu = tot + (size_t)(slot * 3 + cz) * 10240;
        __int128 inner = 0;
#pragma unroll
        for (u32 v = 0; v < 8; v++) {
            const u32 col = (b * 3 + cq) * 8 + v, nt = col >> 4, cl = col & 15;
            inner += (__int128)tu[((size_t)u * 5 + nt) * 256 + (cl + 16 * (av >> 2)) * 4 + (av & 3)] << (8 * v);
        }
        u64 val = fq_from_s128((u64)inner, (int64_t)(inner >> 64));
        u64 pw = 1;
        for (u32 i = 0; i < u; i++) pw = fq_mul(pw, 256);
        val = fq_mul(val, pw);
        if (cz + cq >= 3) val = fq_mul(val, nu);
        sm[t] = val;
    }
    __syncthreads();
    if (t == 0) {
        u64 res = 0;
        for (int i = 0; i < 24; i++) res = fq_add(res, sm[i]);
        out[((size_t)av * nb_out + b0 + b) * 24 + 3 * slot + comp] = fq_canon(res);   // (nb_out, b0: this launch's Y vectors are b0 .. b0 + nb - 1 of nb_out)
    }
}

size_t dot_i8_yb_bytes(size_t n) { return (size_t)8 * 72 * (cdiv(n, 64) * 64) + 64; }
size_t dot_i8_part_words(size_t) { return (size_t)24 * DOT_CHUNKS * 10240; }   // (the largest chunk count: see DotPlan)
size_t dot_i8_tot_words() { return (size_t)24 * 10240; }
// the Y digits alone (k_dot_pack_y), for a following launch_dot_batch_i8(.., y_packed = true) on vectors X with the same alignment: two X sets against the
// same Y (the eta inner products of the two sides of a fold step) pack it once.  Result: lf_i8_launch.h.
int launch_dot_pack_y(const u64 *X, const u64 *Y, size_t ldy, u32 nb, size_t n, unsigned char *YB, hipStream_t s) {
    DotPlan p;
    if (!dot_i8_shape(X, 2, 1, nb, n, &p)) return I8_ERR_SHAPE;   // (the Y side alone: na and ldx are the following launch's)
    hipLaunchKernelGGL((k_dot_pack_y<u64, 3>), dim3(p.pack_blocks(nb, 24)), dim3(256), 0, s, Y - p.lead, ldy, nb, p.n, p.lead, p.ldq, YB);
    return i8_launched();
}
// q_j = M_j^T eq(r) for the nm <= 3 matrices of a step, written ONLY as the packed digits YB that k_dot_i8 reads: the gather of k_spmv_t_eq (lf_kernels.hip: the
// same CSC walk, the same product and the same order of the sums, so the words are the ones that kernel stores) and the digit cut of k_dot_pack_y in one pass --
// the words, 151 MB at 2^18 columns x 3 matrices, are never stored and never read back.
// block = (one K-step block of 64 columns, one matrix: blockIdx.y).  Gather: thread = (column cl of 32, slot) as in k_spmv_t_eq, the two halves of the block in
// turn.  The balanced words cross LDS as sm[word plane][column] (rows of 66 words: the eight slots of a column -- planes 3 apart -- land on eight different
// bank quads, ds_write_b64 conflict-free).  Cut: thread = (word plane, four operand positions 4 q .. 4 q + 3), which hold columns c, c + 1, c + 8, c + 9 with
// c = kstep_col(4 q): two 16-byte LDS reads, and per digit v one 32-bit word (gather_bytes) into digit row v -- 16 lanes store one 64-byte row segment.
// Columns >= n and empty columns give zero digits.
// (All nm matrices in one block -- 38 KB of LDS, 125 to 188 registers, two to four blocks per CU -- took 650 to 720 us next to the commit, on the 32 CUs it leaves,
// where the three k_spmv_t_eq and k_dot_pack_y take 470; with the first non-zero of the six columns of a thread loaded side by side it was no faster.)
struct QPackArgs {
    const u32 *colptr[3], *rowidx[3];
    const u64 *val[3], *eq;
    size_t m, n, ldq;      // ldq: n padded to blocks of 64, the row length of YB
    unsigned char *YB;     // [8][72][ldq]
};
template <bool NU>
__global__ void __launch_bounds__(256) k_q_pack_i8(DevCrt t, QPackArgs a) {
    const u32 cl = threadIdx.x >> 3, slot = threadIdx.x & 7, j = blockIdx.y;
    const size_t cb = (size_t)blockIdx.x * 64;
    __shared__ __attribute__((aligned(16))) u64 sm[24][66];
    const u32 *colptr = a.colptr[j], *rowidx = a.rowidx[j];
    const u64 *val = a.val[j];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const size_t c = cb + 32 * h + cl;
        Fq3 acc = fq3_zero();
        if (c < a.n)
            for (u32 k = colptr[c]; k < colptr[c + 1]; k++) {
                const u64 *v = val + (size_t)k * 24 + 3 * slot;
                const size_t r = rowidx[k];
                acc = fq3_add(acc, fq3_mul<NU>(fq3_make(v[0], v[1], v[2]), fq3_make(a.eq[r], a.eq[a.m + r], a.eq[2 * a.m + r]), t.nu));
            }
#pragma unroll
        for (int cq = 0; cq < 3; cq++) sm[3 * slot + cq][32 * h + cl] = balanced_bytes(acc.c[cq]);
    }
    __syncthreads();
    for (u32 task = threadIdx.x; task < 24 * 16; task += 256) {
        const u32 pos0 = 4 * (task & 15), plane = task >> 4;
        const u32 c = kstep_col(pos0);   // even; positions pos0 + 2, pos0 + 3 hold columns c + 8, c + 9
        const ulonglong2 lo = *(const ulonglong2 *)&sm[plane][c], hi = *(const ulonglong2 *)&sm[plane][c + 8];
        unsigned char *dst = a.YB + ((size_t)(plane / 3) * 72 + (j * 3 + plane % 3) * 8) * a.ldq + cb + pos0;
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const int sh = v < 4 ? 0 : 32;
            *(u32 *)(dst + (size_t)v * a.ldq) = gather_bytes((u32)(lo.x >> sh), (u32)(lo.y >> sh), (u32)(hi.x >> sh), (u32)(hi.y >> sh), v & 3);
        }
    }
}
// The Y digits of q_j = M_j^T eq, j < nm <= 3, for following launch_dot_batch_i8(.., y_packed = true) calls on vectors X of this alignment -- what
// nm x launch_spmv_t_eq + launch_dot_pack_y leave in YB, without the words.  Declines (I8_ERR_SHAPE, nothing launched) where the dot launch would, and where the
// slice needs a lead column (its digits sit one position to the right: the two-pass form handles that).  Result: lf_i8_launch.h.
int launch_q_pack_i8(const DevCrt &t, u32 nm, const u32 *const *colptr, const u32 *const *rowidx, const u64 *const *val, const u64 *eq, size_t m, const u64 *X,
                     size_t n, unsigned char *YB, hipStream_t s) {
    DotPlan p;
    if (!dot_i8_shape(X, 2, 1, nm, n, &p) || p.lead) return I8_ERR_SHAPE;
    QPackArgs a = {};
    for (u32 j = 0; j < nm; j++) { a.colptr[j] = colptr[j]; a.rowidx[j] = rowidx[j]; a.val[j] = val[j]; }
    a.eq = eq; a.m = m; a.n = n; a.ldq = p.ldq; a.YB = YB;
    if (t.nu2p40) hipLaunchKernelGGL(k_q_pack_i8<true>, dim3(p.nsteps, nm), dim3(256), 0, s, t, a);
    else hipLaunchKernelGGL(k_q_pack_i8<false>, dim3(p.nsteps, nm), dim3(256), 0, s, t, a);
    return i8_launched();
}
// X [na][24][ldx], Y [nb][24][ldy], n columns; out[(a*nb + b)*24 + 3*slot + comp] canonical.  Result: lf_i8_launch.h.
int launch_dot_batch_i8(const DevCrt &t, const u64 *X, size_t ldx, u32 na, const u64 *Y, size_t ldy, u32 nb, size_t n, unsigned char *YB, int32_t *part,
                        long long *tot, u64 *out, hipStream_t s, bool y_packed, u32 nb_out, u32 b0) {
    if (!nb_out) nb_out = nb;
    DotPlan p;
    if (!dot_i8_shape(X, ldx, na, nb, n, &p)) return I8_ERR_SHAPE;
    if (!y_packed) hipLaunchKernelGGL((k_dot_pack_y<u64, 3>), dim3(p.pack_blocks(nb, 24)), dim3(256), 0, s, Y - p.lead, ldy, nb, p.n, p.lead, p.ldq, YB);
    const DotI8Args a = p.args<DotI8Args>(X, ldx, na, YB, 24 * nb, part);
    hipLaunchKernelGGL(k_dot_i8, dim3((unsigned)cdiv(a.chunks, 4) * 24), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_dot_sum<10240>, dim3(40, 24), dim3(256), 0, s, part, a.chunks, tot);
    hipLaunchKernelGGL(k_dot_i8_finish, dim3(na * nb * 24), dim3(32), 0, s, tot, na, nb, t.nu, out, nb_out, b0);
    return i8_launched();
}
}  // namespace lf
