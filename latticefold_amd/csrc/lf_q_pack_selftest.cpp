// lf_q_pack_selftest.cpp -- stand-alone host program (make q-pack-selftest, address and undefined-behaviour sanitizers, no GPU, no library):
//   1. the byte placement of the fused gather-and-pack kernel k_q_pack_i8 (lf_dot_i8.hip), restated here from balanced_bytes and kstep_col, against the
//      restatement of k_dot_pack_y (lf_dot_i8.cuh) applied to the same words of q: the two images of YB must be equal byte for byte, for n = 64, 66, 130, 258
//      columns and t = 1, 2, 3 matrices, the rows beyond the t matrices untouched by both;
//   2. the shape test of lf_dot_plan.h (dot_i8_shape / dot_i8_takes) against DotPlan::make and the bounds the launchers used to spell out, over a case table.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lf_dot_plan.h"

using namespace i8mma;
typedef uint64_t u64;
typedef uint32_t u32;
static const u64 P = 0xFFFFFFFF00000001ull;
static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
// canonical words with the corners of balanced_bytes among them: 0, p - 1, the first word that wraps past 2^64, bytes 0x7f / 0x80 everywhere
static u64 word(size_t i) {
    static const u64 corner[] = {0, 1, P - 1, 0x7F7F7F7F7F7F7F7Full, 0x7F7F7F7F7F7F7F80ull, 0x8080808080808080ull, 0xFFFFFFFF00000000ull, 0x00000000FFFFFFFFull, 0x7F7F7F7F80808080ull, 0xFFFFFFFEFFFFFFFFull};
    if (i % 7 == 3) return corner[(i / 7) % (sizeof(corner) / sizeof(corner[0]))];
    return rnd() % P;
}
static long checks = 0, bad = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { if (bad++ < 20) { printf("MISMATCH: " __VA_ARGS__); printf("\n"); } } } while (0)

// k_dot_pack_y<u64, 3> with lead = 0: YB[slot][(b*3 + cq)*8 + v][i0 + pos] = digit v of Y_b[3 slot + cq][i0 + kstep_col(pos)], zero for columns >= n
static void pack_y_host(const std::vector<u64> &q, size_t ldy, u32 nb, size_t n, size_t ldq, std::vector<unsigned char> &YB) {
    for (u32 b = 0; b < nb; b++)
        for (u32 slot = 0; slot < 8; slot++)
            for (u32 cq = 0; cq < 3; cq++)
                for (size_t i0 = 0; i0 < ldq; i0 += 64)
                    for (u32 pos = 0; pos < 64; pos++) {
                        const size_t i = i0 + kstep_col(pos);
                        const u64 w = i < n ? balanced_bytes(q[((size_t)b * 24 + 3 * slot + cq) * ldy + i]) : 0;
                        for (u32 v = 0; v < 8; v++) YB[((size_t)slot * 72 + (b * 3 + cq) * 8 + v) * ldq + i0 + pos] = (unsigned char)(w >> (8 * v));
                    }
}
// k_q_pack_i8: block = (64 columns, matrix j); the balanced words of the block cross sm[word plane][column] (zero for columns >= n); task = (plane, quad):
// positions 4 quad .. 4 quad + 3 hold columns c, c + 1, c + 8, c + 9 with c = kstep_col(4 quad); digit v of the four goes as ONE 32-bit store to row v
// (the blocks of the nm matrices are laid side by side in sm here)
static void q_pack_host(const std::vector<u64> &q, size_t ldy, u32 nm, size_t n, size_t ldq, std::vector<unsigned char> &YB) {
    std::vector<u64> sm((size_t)nm * 24 * 66);
    for (size_t cb = 0; cb < ldq; cb += 64) {
        for (u32 tid = 0; tid < 256; tid++) {
            const u32 cl = tid >> 3, slot = tid & 7;
            for (u32 j = 0; j < nm; j++)
                for (u32 h = 0; h < 2; h++) {
                    const size_t c = cb + 32 * h + cl;
                    for (u32 cq = 0; cq < 3; cq++) sm[((size_t)j * 24 + 3 * slot + cq) * 66 + 32 * h + cl] = balanced_bytes(c < n ? q[((size_t)j * 24 + 3 * slot + cq) * ldy + c] : 0);
                }
        }
        for (u32 task = 0; task < nm * 24 * 16; task++) {
            const u32 pos0 = 4 * (task & 15), plane = (task >> 4) % 24, j = task / (24 * 16);
            const u32 c = kstep_col(pos0);
            const u64 *s = &sm[((size_t)j * 24 + plane) * 66];
            const u64 w[4] = {s[c], s[c + 1], s[c + 8], s[c + 9]};
            unsigned char *dst = &YB[((size_t)(plane / 3) * 72 + (j * 3 + plane % 3) * 8) * ldq + cb + pos0];
            for (u32 v = 0; v < 8; v++) {
                u32 o = 0;   // gather_bytes: byte v of w[0..3] in that order, lowest address first
                for (u32 i = 0; i < 4; i++) o |= (u32)((w[i] >> (8 * v)) & 0xFF) << (8 * i);
                memcpy(dst + (size_t)v * ldq, &o, 4);
            }
        }
    }
}
static void placement() {
    const size_t ns[] = {64, 66, 130, 258};
    for (size_t n : ns)
        for (u32 t = 1; t <= 3; t++) {
            const long before = checks;
            DotPlan p;
            alignas(16) static u64 x[2];
            CHECK(lf::dot_i8_shape(x, n, 16, t, n, &p) && p.lead == 0, "plan n=%zu", n);
            const size_t ldq = (n + 63) / 64 * 64;
            CHECK(p.ldq == ldq && p.nsteps == ldq / 64, "ldq n=%zu", n);
            std::vector<u64> q((size_t)t * 24 * n);
            for (size_t i = 0; i < q.size(); i++) q[i] = word(i);
            // an empty column (all 24 words of every matrix zero)
            for (u32 pl = 0; pl < t * 24; pl++) q[(size_t)pl * n + 5] = 0;
            std::vector<unsigned char> A((size_t)8 * 72 * ldq + 64, 0xA5), B(A);
            pack_y_host(q, n, t, n, ldq, A);
            q_pack_host(q, n, t, n, ldq, B);
            for (size_t i = 0; i < A.size(); i++) CHECK(A[i] == B[i], "n=%zu t=%u byte %zu (slot %zu row %zu pos %zu): pack_y %02x fused %02x", n, t, i, i / (72 * ldq), (i / ldq) % 72, i % ldq, A[i], B[i]);
            // both leave the digit rows of absent matrices and the tail of the buffer alone, and write every byte of the rows they own
            for (u32 slot = 0; slot < 8; slot++)
                for (u32 r = 0; r < 72; r++)
                    for (size_t i = 0; i < ldq; i++) {
                        const unsigned char b = B[((size_t)slot * 72 + r) * ldq + i];
                        if (r >= 24 * t) CHECK(b == 0xA5, "n=%zu t=%u row %u written", n, t, r);
                        else if (i / 64 * 64 + kstep_col((u32)(i % 64)) >= n) CHECK(b == 0, "n=%zu t=%u pad byte %02x", n, t, b);
                    }
            printf("placement n=%zu t=%u: %ld checks ok\n", n, t, checks - before);
        }
}
static void predicate() {
    const long before = checks;
    alignas(16) static u64 buf[4];
    struct Case { size_t off, ldx; u32 na, nb; size_t n; bool shape; size_t lead; };
    const size_t big = (size_t)2047 * 64 * lf::DOT_CHUNKS;   // the last column count at which every wave adds fewer than 2048 K-steps into its int32 accumulators (40 chunks of 2047)
    const Case cases[] = {
        {0, 66, 16, 3, 66, true, 0},   {0, 258, 16, 3, 258, true, 0}, {0, 64, 1, 1, 64, true, 0},  {0, 64, 16, 3, 63, false, 0},   // fewer than 64 columns
        {0, 63, 16, 3, 64, false, 0},  /* odd ldx */                  {0, 66, 17, 3, 66, false, 0}, {0, 66, 0, 3, 66, false, 0},   // na
        {0, 66, 16, 4, 66, false, 0},  {0, 66, 16, 0, 66, false, 0},  /* nb */                      {1, 66, 16, 3, 66, true, 1},    // a slice on an odd word: lead column
        {0, 1 << 18, 16, 3, (size_t)1 << 18, true, 0},                {0, big, 16, 3, big, true, 0}, {0, big + 2, 16, 3, big + 1, false, 0},   // the overflow bound
    };
    for (const Case &c : cases) {
        const u64 *X = buf + c.off;
        DotPlan p, m;
        const bool made = m.make(X, c.n, lf::DOT_CHUNKS);
        const bool spelled = !(c.na < 1 || c.na > 16 || c.nb < 1 || c.nb > 3 || (c.ldx & 1) || !made);   // what launch_dot_batch_i8 used to test
        const bool got = lf::dot_i8_shape(X, c.ldx, c.na, c.nb, c.n, &p);
        CHECK(got == c.shape && got == spelled, "shape off=%zu ldx=%zu na=%u nb=%u n=%zu: %d, table %d, launcher %d", c.off, c.ldx, c.na, c.nb, c.n, got, c.shape, spelled);
        if (got) CHECK(p.lead == c.lead && p.lead == m.lead && p.n == m.n && p.ldq == m.ldq && p.chunks == m.chunks && p.steps_per_chunk == m.steps_per_chunk && p.chunks <= lf::DOT_CHUNKS, "plan n=%zu", c.n);
        // the drivers' gate on top: LF_DOT_VALU and LF_DOT_MIN
        CHECK(lf::dot_i8_takes(false, 4096, X, c.ldx, c.na, c.nb, c.n, &p) == (c.shape && c.n >= 4096), "takes dot_min n=%zu", c.n);
        CHECK(lf::dot_i8_takes(false, 64, X, c.ldx, c.na, c.nb, c.n, &p) == c.shape, "takes n=%zu", c.n);
        CHECK(!lf::dot_i8_takes(true, 64, X, c.ldx, c.na, c.nb, c.n, &p), "takes valu n=%zu", c.n);
    }
    const u64 *mis = (const u64 *)((const char *)buf + 4);   // words not aligned (never dereferenced)
    DotPlan p;
    CHECK(!lf::dot_i8_shape(mis, 66, 16, 3, 66, &p) && !p.make(mis, 66, lf::DOT_CHUNKS), "misaligned words");
    printf("predicate: %ld checks ok\n", checks - before);
}
int main() {
    placement();
    predicate();
    if (bad) { printf("q pack selftest FAILED: %ld of %ld checks\n", bad, checks); return 1; }
    printf("q pack selftest ok: %ld checks\n", checks);
    return 0;
}
