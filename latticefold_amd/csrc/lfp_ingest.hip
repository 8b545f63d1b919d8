// lfp_ingest.hip -- ComR1CS::new (crates/latticefold-plus/src/r1cs.rs:48-60) on the device: f = z.gadget_decompose(b, k), cm_f = A f, one pass over A.
//
// Thread (g = tid >> 4, t = tid & 15) owns coefficient t of z element j = j0 + g of the current tile of 16 elements and keeps its centred value in a
// register; step i of the tile cuts digit i of it (digit_step), which is coefficient t of f row j k + i: the row goes out as canonical words and its
// product with the kappa words A[.][j k + i][.] enters cm_f.  A row of A is used exactly once, by the 16 lanes that loaded it: the tile is exchanged through
// LDS (digits as a +- table of 32 entries, so that the negacyclic wrap is a masked index) and there is no reuse to block for.
//   * every f coefficient is a SIGNED DIGIT, |d| <= b/2 <= 2^30: a term is one 64-bit word times an int32, accumulated as a signed 128-bit integer
//     (|A| < 2^64, 16 terms per row, n <= 2^28 rows: < 2^126, exact), reduced mod p once per block; k_reduce adds the blocks;
//   * loads are whole 128-byte ring elements per 16 lanes; the A words of the next step and the z words of the next tile are in flight while the
//     current step is consumed; f is written with plain vector stores.
#include "lfp_kernels.h"
#include "lfp_dev.cuh"

namespace lfp {
typedef __int128 i128;

// acc += a * d, a an unsigned word, d a signed digit
__device__ __forceinline__ void mac_digit(i128 &acc, u64 a, int32_t d) {
    const int64_t pl = (int64_t)(u64)(u32)a * (int64_t)d, ph = (int64_t)(a >> 32) * (int64_t)d;     // |.| < 2^62 each
    acc += (i128)pl + ((i128)ph << 32);
}
// the signed sum mod p
__device__ __forceinline__ u64 mod_p_i128(i128 x) {
    const bool neg = x < 0;
    const unsigned __int128 mag = neg ? (unsigned __int128)(-x) : (unsigned __int128)x;
    const u64 r = red_word((u64)(mag >> 64) % P, (u64)mag);
    return neg && r ? P - r : r;
}

template <int ICNT>
__global__ __launch_bounds__(256) void k_ingest(IngestArgs a) {
    __shared__ u64 atab[2][ICNT][16][16];
    __shared__ int32_t dtab[2][16][32];      // [d_0 .. d_15, -d_0 .. -d_15] per row
    __shared__ u64 red[4][16];
    const int tid = threadIdx.x, t = tid & 15, g = tid >> 4;
    const u64 jb = (u64)blockIdx.x * a.JZ;
    const u64 jend = jb + a.JZ < a.m ? jb + a.JZ : a.m;
    i128 acc[ICNT];
#pragma unroll
    for (int i = 0; i < ICNT; i++) acc[i] = 0;

    u64 zn = jb + g < jend ? a.z[(jb + g) * D + t] : 0, an[ICNT];
#pragma unroll
    for (int i = 0; i < ICNT; i++) an[i] = jb + g < jend ? a.A[((u64)(a.i0 + i) * a.n + (jb + g) * a.k) * D + t] : 0;
    int p = 0;
    for (u64 j0 = jb; j0 < jend; j0 += 16) {
        const u64 j = j0 + g;
        const bool in = j < jend;
        const u64 zv = zn;
        zn = j + 16 < jend ? a.z[(j + 16) * D + t] : 0;
        if (a.first && zv >= P) atomicOr(a.err, 4u);
        int64_t cur = centre(zv);
        for (u32 i = 0; i < a.k; i++) {
            u64 av[ICNT];
#pragma unroll
            for (int q = 0; q < ICNT; q++) av[q] = an[q];
            {   // the A words of the next step: digit i + 1 of this element, or digit 0 of the next tile's
                const bool last = i + 1 == a.k;
                const u64 rn = last ? (j + 16) * a.k : j * a.k + i + 1;
                const bool okn = last ? j + 16 < jend : in;
#pragma unroll
                for (int q = 0; q < ICNT; q++) an[q] = okn ? a.A[((u64)(a.i0 + q) * a.n + rn) * D + t] : 0;
            }
            const int32_t d = (int32_t)digit_step(cur, a.b, a.sh);      // (zv = 0 outside the range: d = 0)
            if (a.first && in) a.f[(j * a.k + i) * D + t] = d >= 0 ? (u64)d : P - (u64)(-(int64_t)d);
            dtab[p][g][t] = d;
            dtab[p][g][16 + t] = -d;
#pragma unroll
            for (int q = 0; q < ICNT; q++) atab[p][q][g][t] = av[q];
            __syncthreads();      // (one barrier per step: the step after the next is the first to write this buffer again)
#pragma unroll 4      // (fully unrolled the compiler hoists all 16 LDS reads of every row: 300+ VGPRs, one wave per SIMD)
            for (int s = 0; s < D; s++) {
                const int32_t dv = dtab[p][g][(t - s) & 31];
#pragma unroll
                for (int q = 0; q < ICNT; q++) mac_digit(acc[q], atab[p][q][g][s], dv);
            }
            p ^= 1;
        }
    }
    u64 *part = a.part + (u64)blockIdx.x * a.kappa * D;
#pragma unroll
    for (int q = 0; q < ICNT; q++) {
        const u64 r = sum_over_row_lanes(mod_p_i128(acc[q]), red, tid);
        if (tid < 16) part[(a.i0 + q) * D + tid] = r;
    }
}

hipError_t launch_ingest(const IngestArgs &a, u32 nblk, hipStream_t s) {
    if (a.icnt == 1) hipLaunchKernelGGL(k_ingest<1>, dim3(nblk), dim3(256), 0, s, a);
    else if (a.icnt == 2) hipLaunchKernelGGL(k_ingest<2>, dim3(nblk), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_ingest<4>, dim3(nblk), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- the seeded commitment matrix (lfplus_matrix_generate; the host form is PlusWorkload.ajtai_matrix) -----------------------------------------------
// Word w of the row-major (kappa, n, 16) matrix is splitmix64(seed + (w + 1) G) mod p: an indexable stream, so every word is independent of the others and the
// kernel is a pure write stream.  2^64 < 2 p: the reduction is one conditional subtraction.  A thread writes two consecutive words with one 16-byte store (the
// total is a multiple of 16 words and the buffer a device allocation: every pair is 16-byte aligned); the grid strides over the pairs with a 64-bit index.
__device__ __forceinline__ u64 ajtai_word(u64 seed, u64 w) {
    u64 z = seed + (w + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z >= P ? z - P : z;
}
__global__ __launch_bounds__(256) void k_fill_ajtai(u64 *out, u64 pairs, u64 seed) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < pairs; q += stride) {
        ulonglong2 v;
        v.x = ajtai_word(seed, 2 * q);
        v.y = ajtai_word(seed, 2 * q + 1);
        reinterpret_cast<ulonglong2 *>(out)[q] = v;
    }
}
hipError_t launch_fill_ajtai(u64 *out, u64 words, u64 seed, hipStream_t s) {
    const u64 pairs = words / 2;      // (words is a multiple of 16)
    if (!pairs) return hipSuccess;
    const u64 want = (pairs + 255) / 256;
    const u32 nblk = (u32)(want < 16384 ? want : 16384);      // 64 blocks per CU: enough stores in flight to fill HBM, few enough that the tail is short
    hipLaunchKernelGGL(k_fill_ajtai, dim3(nblk), dim3(256), 0, s, out, pairs, seed);
    return hipGetLastError();
}
}  // namespace lfp
