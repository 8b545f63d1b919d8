// bb_dot_i8.hip -- BabyBear: batched inner products of F_{p^9}-slot vectors on the int8 matrix cores (the BabyBear form of lf_dot_i8.hip):
//     out[a][b][slot] = sum_i X_a[slot][i] * Y_b[slot][i]        (a < na <= 16 vectors X, b < nb <= 3 vectors Y, 8 slots, n columns)
// -- u_s and eta of a fold step (<z_k, M_j^T eq(r)>), was lfbb::k_dot_batch: 27 F_{p^9} products per column and slot on v_mad_i64_i32.
//
// A residue is a centred Montgomery word x~ in [-H, H], H < 2^30 (bb_field.cuh).  Its four balanced base-256 digits d_u in [-128, 127],
// sum_u d_u 256^u = x~, are the bytes of (x~ + 0x80808080) ^ 0x80808080, so sum_i x~ y~ = sum_{u,v} 256^(u+v) sum_i d_u e_v: per
// (slot, component cx of X) an exact int8 GEMM with rows = (digit u, vector a) -- 4 row tiles --, inner dimension = columns, matrix columns =
// (vector b, component cy, digit v) of Y -- 108 = 7 column tiles.  X digits are cut in registers from coalesced loads (one instruction = 32
// contiguous bytes per vector row), Y digits are packed once per call in the same inner-dimension order.  The finish undoes the two
// Montgomery factors (sum x~ y~ = R^2 sum x y), applies Y^9 = nu and reduces mod p.
#include <hip/hip_runtime.h>
#include "bb_field.cuh"
#include "bb_kernels.h"
#include "lf_dot_i8.cuh"

namespace lfbb {
using namespace i8mma;

struct BbDotArgs : DotArgs<fe> {};   // X [na][72][ldx], YB [8][108][ldq], part [unit 72][chunk][u 4][nt 7][64][4]

// wave = one (slot, cx) unit x one chunk of columns; the loads of the next K-step are in flight while this one is computed (two operand buffers; lf::k_dot_i8
// rotates three: see the note there)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_bbdot_i8(BbDotArgs a) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, g = lane >> 4;
    const u32 unit = blockIdx.y, slot = unit / TAU, cx = unit % TAU;
    const u32 chunk = blockIdx.x * 4 + wave;
    v4i acc[4][7];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int nt = 0; nt < 7; nt++) acc[u][nt] = v4i{0, 0, 0, 0};
    if (chunk >= a.chunks) return;
    const u32 s0 = chunk * a.steps_per_chunk, s1 = s0 + a.steps_per_chunk < a.nsteps ? s0 + a.steps_per_chunk : a.nsteps;
    const fe *xrow = a.X + ((size_t)row * RE + TAU * slot + cx) * a.ldx;
    const bool xlive = row < a.na;
    const unsigned char *yb = a.YB + (size_t)slot * 108 * a.ldq;
    const u32 last = s1 > s0 ? s1 - 1 : s0;
    u32 xa[16], xn[16];
    v4i ba[7], bn[7];
    dot_load_x(xrow, (size_t)s0 * 64, g, a.n, xlive, xa); dot_load_y(yb, a.ldq, (size_t)s0 * 64 + 16 * g, row, a.nrows_y, ba);
    for (u32 st = s0; st < s1; st++) {
        const size_t iwn = (size_t)(st + 1 < last ? st + 1 : last) * 64;
        dot_load_x(xrow, iwn, g, a.n, xlive, xn); dot_load_y(yb, a.ldq, iwn + 16 * g, row, a.nrows_y, bn);
        u32 w[16];
#pragma unroll
        for (int t = 0; t < 16; t++) w[t] = balanced_bytes(xa[t]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            u32 op[4];
#pragma unroll
            for (int j = 0; j < 4; j++) op[j] = gather_bytes(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3], u);
            const v4i av = v4i{(int)op[0], (int)op[1], (int)op[2], (int)op[3]};
#pragma unroll
            for (int nt = 0; nt < 7; nt++) acc[u][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, ba[nt], acc[u][nt], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 16; t++) xa[t] = xn[t];
#pragma unroll
        for (int nt = 0; nt < 7; nt++) ba[nt] = bn[nt];
    }
    int32_t *o = a.part + ((size_t)unit * a.chunks + chunk) * (4 * 7 * 256);
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int nt = 0; nt < 7; nt++) *(v4i *)(o + ((size_t)u * 7 + nt) * 256 + lane * 4) = acc[u][nt];
}
// block = output (a, b, slot, c), thread = (cx, digit u): out[(a*nb + b)*72 + 9*slot + c] = canonical of
//   R^-2 * sum over (cx, cy) with cx + cy = c (mod 9) of nu^[cx+cy >= 9] * sum_{u,v} 256^(u+v) tot[slot, cx][u][a][(b, cy, v)]
__global__ void __launch_bounds__(64) k_bbdot_finish(const long long *tot, u32 na, u32 nb, u32 nu_canon, u32 rinv2, u64 *out) {
    __shared__ u64 sm[36];
    const u32 o = blockIdx.x, t = threadIdx.x;
    const u32 c = o % TAU, slot = (o % RE) / TAU, b = (o / RE) % nb, av = o / (RE * nb);
    const u64 P = BB_P;
    if (t < 36) {
        const u32 cx = t >> 2, u = t & 3, cy = (c + TAU - cx) % TAU;
        const long long *tu = tot + (size_t)(slot * TAU + cx) * 7168;
        u64 val = 0, pw = 1;
        for (u32 v = 0; v < 4; v++) {
            const u32 col = (b * TAU + cy) * 4 + v, nt = col >> 4, cl = col & 15;
            const long long cell = tu[((size_t)u * 7 + nt) * 256 + (cl + 16 * (av >> 2)) * 4 + (av & 3)];
            const u64 cm = (u64)((cell % (long long)P + (long long)P) % (long long)P);
            val = (val + cm * pw) % P;
            pw = pw * 256 % P;
        }
        u64 pu = 1;
        for (u32 i = 0; i < u; i++) pu = pu * 256 % P;
        val = val * pu % P;
        if (cx + cy >= TAU) val = val * nu_canon % P;
        sm[t] = val;
    }
    __syncthreads();
    if (t == 0) {
        u64 res = 0;
        for (int i = 0; i < 36; i++) res = (res + sm[i]) % P;
        out[o] = res * rinv2 % P;
    }
}

size_t bbdot_i8_yb_bytes(size_t n) { return (size_t)8 * 108 * (cdiv(n, 64) * 64) + 64; }
constexpr u32 BBDOT_CHUNKS = 12;   // 72 units x 12 chunks = 216 blocks of 4 waves: one batch on 256 CUs at one wave per SIMD
size_t bbdot_i8_part_words(size_t) { return (size_t)72 * BBDOT_CHUNKS * 7168; }   // (the largest chunk count: see DotPlan)
size_t bbdot_i8_tot_words() { return (size_t)72 * 7168; }
static u64 bb_powmod(u64 a, u64 e) {
    u64 r = 1;
    a %= BB_P;
    while (e) { if (e & 1) r = r * a % BB_P; a = a * a % BB_P; e >>= 1; }
    return r;
}
// the Y digits alone, for launch_dot_batch_i8(.., y_packed = true) calls on X vectors of the same alignment (the eta products of the two sides of a fold step).
// Result: lf_i8_launch.h.
int launch_dot_pack_y(const fe *X, const fe *Y, size_t ldy, u32 nb, size_t n, unsigned char *YB, hipStream_t s) {
    DotPlan p;
    if (nb < 1 || nb > 3 || !p.make(X, n, BBDOT_CHUNKS)) return I8_ERR_SHAPE;
    hipLaunchKernelGGL((k_dot_pack_y<fe, TAU>), dim3(p.pack_blocks(nb, RE)), dim3(256), 0, s, Y - p.lead, ldy, nb, p.n, p.lead, p.ldq, YB);
    return i8_launched();
}
// X [na][72][ldx], Y [nb][72][ldy] (centred Montgomery words), n columns; out[(a*nb + b)*72 + 9*slot + c] canonical.  Result: lf_i8_launch.h.
int launch_dot_batch_i8(const DevBb &t, const fe *X, size_t ldx, u32 na, const fe *Y, size_t ldy, u32 nb, size_t n, unsigned char *YB, int32_t *part,
                        long long *tot, u64 *out, hipStream_t s, bool y_packed) {
    DotPlan p;
    if (na < 1 || na > 16 || nb < 1 || nb > 3 || (ldx & 1) || !p.make(X, n, BBDOT_CHUNKS)) return I8_ERR_SHAPE;
    if (!y_packed) hipLaunchKernelGGL((k_dot_pack_y<fe, TAU>), dim3(p.pack_blocks(nb, RE)), dim3(256), 0, s, Y - p.lead, ldy, nb, p.n, p.lead, p.ldq, YB);
    const BbDotArgs a = p.args<BbDotArgs>(X, ldx, na, YB, 36 * nb, part);
    hipLaunchKernelGGL(k_bbdot_i8, dim3((unsigned)cdiv(a.chunks, 4), 72), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_dot_sum<7168>, dim3(28, 72), dim3(256), 0, s, part, a.chunks, tot);
    const u64 rinv = bb_powmod(BB_R, BB_P - 2);
    hipLaunchKernelGGL(k_bbdot_finish, dim3(na * nb * RE), dim3(64), 0, s, tot, na, nb, (u32)to_canon(t.nu), (u32)(rinv * rinv % BB_P), out);
    return i8_launched();
}

// ---- T[k][c] = sum_i eq[i] * digit_k(planes[c][i]) (v_s of a decomposition, the linearization's v) on the matrix cores -------------------------------
// The BabyBear form of lf::k_coef_eval_i8 (binary digit planes only): per coefficient c an exact int8 GEMM with rows = the K <= 16 planes (digits -1, 0, 1 cut
// from the int32 plane words in registers), inner dimension = columns, matrix columns = the 36 balanced base-256 digits of the nine words of eq (packed once
// per call).  Was lfbb::k_coef_eval: K * 9 masked 64-bit additions per column and coefficient on the VALU (0.65 ms per call at C3).
__global__ void __launch_bounds__(256) k_bbce_pack_eq(const fe *eq, size_t ldeq, size_t n, size_t ldb, unsigned char *EB) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;     // four columns per thread
    const u32 q = blockIdx.y;
    if (i0 >= ldb) return;
    u32 d[4];
#pragma unroll
    for (int t = 0; t < 4; t++) d[t] = i0 + t < n ? balanced_bytes((u32)eq[(size_t)q * ldeq + i0 + t]) : 0;
#pragma unroll
    for (int u = 0; u < 4; u++)
        *(u32 *)(EB + (size_t)(4 * q + u) * ldb + i0) = ((d[0] >> (8 * u)) & 0xFF) | (((d[1] >> (8 * u)) & 0xFF) << 8) | (((d[2] >> (8 * u)) & 0xFF) << 16) | (((d[3] >> (8 * u)) & 0xFF) << 24);
}
struct BbCeArgs {
    const int32_t *planes;      // [72][ldp]
    size_t ldp, n;
    const unsigned char *EB;    // [36][ldb]
    size_t ldb;
    u32 rows;                   // K <= 16
    u32 steps_per_wg;
    int32_t *part;              // [wg][72][3][64][4]
};
__device__ __forceinline__ int bbce_digit(int32_t v, u32 k) {
    const u32 m = v < 0 ? 0u - (u32)v : (u32)v;
    const int d = (int)((m >> k) & 1);
    return v < 0 ? -d : d;
}
// grid (workgroups over the columns, 3 groups of 24 coefficients); wave w of a workgroup owns the coefficients 24 y + 6 w .. + 5
__global__ void __launch_bounds__(256) k_bbce_i8(BbCeArgs a) {
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, g = lane >> 4;
    const size_t nsteps = (a.n + 63) / 64;
    const size_t s0 = (size_t)blockIdx.x * a.steps_per_wg, s1 = s0 + a.steps_per_wg < nsteps ? s0 + a.steps_per_wg : nsteps;
    v4i acc[6][3];
#pragma unroll
    for (int mi = 0; mi < 6; mi++)
#pragma unroll
        for (int nt = 0; nt < 3; nt++) acc[mi][nt] = v4i{0, 0, 0, 0};
    const bool full16 = (a.ldp & 3) == 0 && (((size_t)a.planes) & 15) == 0;
    for (size_t st = s0; st < s1; st++) {
        const size_t j0 = st * 64 + 16 * g;           // this lane's 16 columns (EB is zero-padded to ldb, a multiple of 64)
        v4i b[3];
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            const u32 r = 16 * nt + row;
            b[nt] = r < 36 ? *(const v4i *)(a.EB + (size_t)r * a.ldb + j0) : v4i{0, 0, 0, 0};
        }
#pragma unroll
        for (int mi = 0; mi < 6; mi++) {
            const u32 c = 24 * blockIdx.y + wave * 6 + mi;
            const int32_t *pl = a.planes + (size_t)c * a.ldp + j0;
            int32_t v[16];
            if (full16 && j0 + 16 <= a.n) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    int4 w = *(const int4 *)(pl + 4 * q);
                    v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 16; q++) v[q] = j0 + q < a.n ? pl[q] : 0;
            }
            u32 w4[4] = {0, 0, 0, 0};
            if (row < a.rows) {
#pragma unroll
                for (int q = 0; q < 16; q++) w4[q >> 2] |= (u32)(unsigned char)bbce_digit(v[q], row) << (8 * (q & 3));
            }
            const v4i av = v4i{(int)w4[0], (int)w4[1], (int)w4[2], (int)w4[3]};
#pragma unroll
            for (int nt = 0; nt < 3; nt++) acc[mi][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b[nt], acc[mi][nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mi = 0; mi < 6; mi++) {
        const u32 c = 24 * blockIdx.y + wave * 6 + mi;
#pragma unroll
        for (int nt = 0; nt < 3; nt++) *(v4i *)(a.part + ((((size_t)blockIdx.x * 72 + c) * 3 + nt) * 64 + lane) * 4) = acc[mi][nt];
    }
}
// block = 64 outputs x 4 groups of workgroups (a thread walks a quarter of the partial buffers; one thread per output: 61 us of serial adds at 256 workgroups)
__global__ void __launch_bounds__(256) k_bbce_sum(const int32_t *part, u32 nwg, long long *tot) {
    const size_t per = (size_t)72 * 3 * 256, i = (size_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const u32 g = threadIdx.x >> 6;
    __shared__ long long sm[4][64];
    long long s = 0;
    if (i < per)
        for (u32 w = g; w < nwg; w += 4) s += part[(size_t)w * per + i];
    sm[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && i < per) tot[i] = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
}
// out[(k*72 + c)*9 + q] canonical: sum_u 256^u C[k][4q + u] is the Montgomery word of the evaluation (integer scaling keeps the Montgomery form)
__global__ void __launch_bounds__(256) k_bbce_finish(const long long *tot, u32 K, u32 rinv, u64 *out) {
    const u32 o = blockIdx.x * 256 + threadIdx.x;
    if (o >= K * 72 * 9) return;
    const u32 q = o % 9, c = (o / 9) % 72, k = o / (9 * 72);
    long long v = 0;
#pragma unroll
    for (u32 u = 0; u < 4; u++) {
        const u32 col = 4 * q + u, nt = col >> 4, cl = col & 15, ln = cl + 16 * (k >> 2), reg = k & 3;
        v += tot[(((size_t)c * 3 + nt) * 64 + ln) * 4 + reg] << (8 * u);      // |tot| <= n * 128: < 2^57 for n < 2^26
    }
    const long long Pm = (long long)BB_P;
    out[o] = (u64)((v % Pm + Pm) % Pm) * rinv % BB_P;      // Montgomery word -> canonical: times 2^-32
}
size_t coef_eval_i8_eb_bytes(size_t n) { return 36 * (cdiv(n, 64) * 64) + 64; }
size_t coef_eval_i8_part_words(u32 nwg) { return (size_t)nwg * 72 * 3 * 256; }
size_t coef_eval_i8_tot_words() { return (size_t)72 * 3 * 256; }
// planes [72][ldp] (n columns), eq [9][ldeq]; K <= 16 binary digit planes.  out[(k*72 + c)*9 + q] canonical (the layout of launch_coef_eval, mode_bits).
// Result: lf_i8_launch.h (shape not handled: the caller keeps lfbb::k_coef_eval).
int launch_coef_eval_i8(const int32_t *planes, size_t ldp, size_t n, const fe *eq, size_t ldeq, u32 K, unsigned char *EB, u32 nwg, int32_t *part, long long *tot,
                        u64 *out, hipStream_t s) {
    if (!n || K < 1 || K > 16 || n >= ((size_t)1 << 26) || (((size_t)EB) & 15)) return I8_ERR_SHAPE;
    const size_t ldb = cdiv(n, 64) * 64, nsteps = ldb / 64;
    hipLaunchKernelGGL(k_bbce_pack_eq, dim3((unsigned)cdiv(ldb / 4, 256), 9), dim3(256), 0, s, eq, ldeq, n, ldb, EB);
    if (nwg > nsteps) nwg = (u32)nsteps;
    BbCeArgs a;
    a.planes = planes; a.ldp = ldp; a.n = n; a.EB = EB; a.ldb = ldb; a.rows = K; a.part = part;
    a.steps_per_wg = (u32)cdiv(nsteps, nwg);
    const u32 grid = (u32)cdiv(nsteps, a.steps_per_wg);
    hipLaunchKernelGGL(k_bbce_i8, dim3(grid, 3), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_bbce_sum, dim3((unsigned)cdiv((size_t)72 * 3 * 256, 64)), dim3(256), 0, s, part, grid, tot);
    hipLaunchKernelGGL(k_bbce_finish, dim3((unsigned)cdiv((size_t)K * 72 * 9, 256)), dim3(256), 0, s, tot, K, (u32)bb_powmod(BB_R, BB_P - 2), out);
    return i8_launched();
}
}  // namespace lfbb
