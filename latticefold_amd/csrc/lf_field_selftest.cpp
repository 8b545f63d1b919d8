// lf_field_selftest.cpp -- the HOST side of lf_field.cuh against `unsigned __int128 %`, as a stand-alone program for a sanitizer build (`make field-selftest`):
// every reduction corner of the Goldilocks code (borrow / carry / hl == 0 of fq_reduce128_loose, the two wraps of fq_from_s128, loose results in [p, 2^64)) is
// reached by the 22-value edge grid below (tests/field_corners.py: EDGE_G), which pseudo-random operands never do.  The undefined-behaviour sanitizer turns a
// signed overflow in the (L, H) accumulators into a failure, so the lazy sums are run up to the largest per-thread product count a launch can reach.
// No GPU is needed.  Prints one line per group and "selftest ok"; exit status 0 only when every group agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lf_field.cuh"

using namespace lf;
typedef unsigned __int128 u128;
typedef __int128 i128;
static const u64 P = 0xFFFFFFFF00000001ULL;

// ---- the reference: plain 128-bit arithmetic and %, nothing from lf_field.cuh ----
static u64 radd(u64 a, u64 b) { return (u64)(((u128)a + b) % P); }
static u64 rsub(u64 a, u64 b) { return (u64)(((u128)a + P - b % P) % P); }
static u64 rmul(u64 a, u64 b) { return (u64)(((u128)(a % P) * (b % P)) % P); }
static u64 rsigned(i128 v) { i128 r = v % (i128)P; return (u64)(r < 0 ? r + (i128)P : r); }
struct R3 { u64 c[3]; };
static R3 rmul3(const R3 &a, const R3 &b, u64 nu) {
    u64 col[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) col[i + j] = radd(col[i + j], rmul(a.c[i], b.c[j]));
    R3 r;
    r.c[0] = radd(col[0], rmul(nu, col[3]));
    r.c[1] = radd(col[1], rmul(nu, col[4]));
    r.c[2] = col[2];
    return r;
}
static R3 radd3(const R3 &a, const R3 &b) { R3 r; for (int i = 0; i < 3; i++) r.c[i] = radd(a.c[i], b.c[i]); return r; }
static R3 rscale3(const R3 &a, u64 k) { R3 r; for (int i = 0; i < 3; i++) r.c[i] = rmul(a.c[i], k); return r; }

static const u64 GRID[22] = {0, 1, 2, P - 1, P - 2, 0xFFFFFFFFULL, 1ULL << 32, (1ULL << 32) + 1, (1ULL << 32) + 2, P - 0xFFFFFFFFULL, 0xFFFFFFFEULL,
                             (P - 1) / 2, (P + 1) / 2, 1ULL << 63, (1ULL << 63) + 1, 1ULL << 40, 1ULL << 24, P - (1ULL << 40), 0xFFFFFFFE00000001ULL,
                             3ULL << 62, 0x1FFFFFFFFULL, P - (1ULL << 24)};
static const int NG = 22;
static const u64 NU40 = 1ULL << 40;
static const u64 NU_GEN = 0xFFFFFFFE00000002ULL;      // a generic constant: fq3_mul<false> is checked as arithmetic, whether or not Y^3 - nu is irreducible

static int fails = 0;
static void group(const char *name, unsigned long long checks, unsigned long long bad) {
    printf("%-44s %10llu checks %s\n", name, checks, bad ? "MISMATCH" : "ok");
    if (bad) { printf("  %llu mismatching words\n", bad); fails++; }
}
static Fq3 f3(const R3 &a) { return fq3_make(a.c[0], a.c[1], a.c[2]); }
static bool same(const Fq3 &a, const R3 &b) { return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2]; }
static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u64 rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
// operand triples: the rotations that put every grid pair into every coordinate position (tests/field_corners.py: all_pairs), then grid triples drawn at random
static void triple(int x, int sh, R3 &a, int m1, int m2) { a.c[0] = GRID[x]; a.c[1] = GRID[(x + m1 * sh) % NG]; a.c[2] = GRID[(x + m2 * sh) % NG]; }

// the value of an AccP from its definition (lf_field.cuh: s00 + s01 2^32 + s11 2^64 + c00 2^64 + c01 2^96 + c11 2^128)
static u64 accp_value(const AccP &s) {
    const u64 t32 = 1ULL << 32, t64 = rmul(t32, t32), t96 = rmul(t64, t32), t128 = rmul(t64, t64);
    u64 r = s.s00 % P;
    r = radd(r, rmul(s.s01, t32));
    r = radd(r, rmul(s.s11, t64));
    r = radd(r, rmul(s.c00, t64));
    r = radd(r, rmul(s.c01, t96));
    r = radd(r, rmul(s.c11, t128));
    return r;
}
static u64 lh_value(const LH &v) { return rsigned((i128)v.l + ((i128)v.h * ((i128)1 << 32))); }

static void test_fp() {
    unsigned long long n = 0, bad = 0;
    for (int i = 0; i < NG; i++) {
        const u64 a = GRID[i];
        bad += fq_neg(a) != rsub(0, a); n++;
        bad += fq_mul_2p40(a) != rmul(a, NU40); n++;
        bad += fq_canon(a) != a; n++;
        for (int j = 0; j < NG; j++) {
            const u64 b = GRID[j];
            bad += fq_add(a, b) != radd(a, b);
            bad += fq_sub(a, b) != rsub(a, b);
            bad += fq_mul(a, b) != rmul(a, b);
            const u128 pr = (u128)a * b;
            const u64 loose = fq_reduce128_loose((u64)pr, (u64)(pr >> 64));
            bad += loose % P != rmul(a, b);
            // any (lo, hi), canonical or not
            bad += fq_reduce128_loose(a, b) % P != radd(rmul(b, (u64)(((u128)1 << 64) % P)), a % P);
            bad += fq_reduce128_loose(~a, ~b) % P != radd(rmul(~b, (u64)(((u128)1 << 64) % P)), (~a) % P);
            n += 6;
        }
    }
    group("fq_add fq_sub fq_neg fq_mul fq_mul_2p40 reduce128", n, bad);
    n = bad = 0;
    const int64_t small[] = {0, 1, -1, 2, -2, 0x7FFFFFFF, -0x7FFFFFFF, 1LL << 32, -(1LL << 32), (1LL << 40) + 3, -((1LL << 40) + 3), INT64_MAX, -INT64_MAX};
    for (int64_t v : small) { bad += fq_from_i64(v) != rsigned(v); n++; }
    group("fq_from_i64", n, bad);
    n = bad = 0;
    const int64_t his[] = {0, 1, -1, 2, -2, 255, -255, (1LL << 29), -(1LL << 29), (1LL << 30) - 1, -((1LL << 30) - 1)};
    for (int i = 0; i < 2 * NG + 4; i++) {
        const u64 lo = i < NG ? GRID[i] : i < 2 * NG ? ~GRID[i - NG] : i == 2 * NG ? ~0ULL : i == 2 * NG + 1 ? P : i == 2 * NG + 2 ? P + 1 : ~0ULL - 0xFFFFFFFFULL;
        for (int64_t hi : his) { bad += fq_from_s128(lo, hi) != rsigned((i128)lo + (i128)hi * ((i128)1 << 64)); n++; }
    }
    for (int i = 0; i < NG; i++)
        for (int j = 0; j < NG; j++) {
            // the linear forms fq3_from_columns_2p40 feeds: small signed base / h32 / h40 (|.| < 2^40)
            const int64_t base = (int64_t)(GRID[i] >> 25) - (int64_t)(GRID[j] >> 24), h32 = (int64_t)(GRID[j] >> 26), h40 = (int64_t)(GRID[i] >> 27) - (int64_t)(GRID[j] >> 26);
            const u64 want = rsigned((i128)base + (i128)h32 * ((i128)1 << 32) + (i128)h40 * ((i128)1 << 40));
            bad += fq_from_lin(base, h32, h40) != want;
            bad += fq_from_lin_wide(base, h32, h40) != want;
            const int64_t k20 = 1 << 20;      // the sizes lazy sums reach
            bad += fq_from_lin_wide(base * k20, h32 * k20, -(h40 * k20)) != rsigned((i128)(base * k20) + (i128)(h32 * k20) * ((i128)1 << 32) - (i128)(h40 * k20) * ((i128)1 << 40));
            n += 3;
        }
    group("fq_from_s128 fq_from_lin fq_from_lin_wide", n, bad);
}

static void test_acc() {
    unsigned long long n = 0, bad = 0;
    for (int i = 0; i < NG; i++)
        for (int j = 0; j < NG; j++) {
            Acc s;
            AccP q;
            acc_set(s, GRID[i], GRID[j]);
            accp_set(q, GRID[i], GRID[j]);
            u64 want = rmul(GRID[i], GRID[j]);
            bad += acc_reduce(s) != want;
            bad += accp_reduce(q) != want || accp_value(q) != want || lh_value(accp_lh(q)) != want;
            // 24 terms (the CRT's row sums): the carry counter of Acc and all three of AccP become non-zero
            for (int k = 1; k < 24; k++) {
                const u64 x = GRID[(i + k) % NG], y = GRID[(j + 5 * k) % NG];
                acc_mad(s, x, y);
                accp_mad(q, x, y);
                want = radd(want, rmul(x, y));
                bad += acc_reduce(s) != want;
                bad += accp_reduce(q) != want || accp_value(q) != want || lh_value(accp_lh(q)) != want;
                n += 4;
            }
        }
    group("acc_set acc_mad acc_reduce accp_* accp_lh", n, bad);
    n = bad = 0;
    unsigned long long ov = 0, c00 = 0, c01 = 0, c11 = 0;
    {   // 24 x (p-1)^2: the counters of the run above, reported
        Acc s; AccP q;
        acc_set(s, P - 1, P - 1); accp_set(q, P - 1, P - 1);
        for (int k = 1; k < 24; k++) { acc_mad(s, P - 1, P - 1); accp_mad(q, P - 1, P - 1); }
        ov = s.ov; c00 = q.c00; c01 = q.c01; c11 = q.c11;
        bad += acc_reduce(s) != 24 || accp_reduce(q) != 24; n += 2;
    }
    const u32 cs[] = {0, 1, 2, 23, 0xFFFF, 0x7FFFFFFF, 0xFFFFFFFFu};
    const u64 ss[] = {0, 1, 0xFFFFFFFFULL, 1ULL << 32, P - 1, P, ~0ULL};
    for (u32 a : cs) for (u32 b : cs) for (u32 c : cs)
        for (u64 x : ss) for (u64 y : ss) for (u64 z : ss) {
            AccP q; q.s00 = x; q.s01 = y; q.s11 = z; q.c00 = a; q.c01 = b; q.c11 = c;
            bad += accp_reduce(q) != accp_value(q); n++;
            if (a < (1u << 31) && b < (1u << 31) && c < (1u << 31)) { bad += lh_value(accp_lh(q)) != accp_value(q); n++; }
        }
    printf("  (24 x (p-1)^2: Acc.ov = %llu, AccP c00 / c01 / c11 = %llu / %llu / %llu)\n", ov, c00, c01, c11);
    group("accp_reduce / accp_lh with set counters", n, bad);
}

static void test_fq3() {
    unsigned long long n = 0, bad = 0;
    auto one = [&](const R3 &a, const R3 &b) {
        bad += !same(fq3_mul<true>(f3(a), f3(b), NU40), rmul3(a, b, NU40));
        bad += !same(fq3_mul<false>(f3(a), f3(b), NU40), rmul3(a, b, NU40));
        bad += !same(fq3_mul<false>(f3(a), f3(b), NU_GEN), rmul3(a, b, NU_GEN));
        bad += !same(fq3_sqr<false>(f3(a), NU_GEN), rmul3(a, a, NU_GEN));
        n += 4;
    };
    for (int sh = 0; sh < 3; sh++)
        for (int i = 0; i < NG; i++)
            for (int j = 0; j < NG; j++) {
                R3 a, b;
                triple(i, sh, a, 1, 2); triple(j, sh, b, 5, 7);
                one(a, b);
            }
    for (int k = 0; k < 20000; k++) {
        R3 a, b;
        for (int q = 0; q < 3; q++) { a.c[q] = GRID[rng() % NG]; b.c[q] = GRID[rng() % NG]; }
        one(a, b);
    }
    // named regression operands: every word p - 1, and the halves
    const R3 m1 = {{P - 1, P - 1, P - 1}}, hf = {{(P - 1) / 2, (P + 1) / 2, (P - 1) / 2}};
    one(m1, m1); one(m1, hf); one(hf, hf);
    group("fq3_mul<true> fq3_mul<false> (2^40, generic) fq3_sqr", n, bad);
}

static void test_lh5() {
    unsigned long long n = 0, bad = 0;
    for (int i = 0; i < NG; i++)
        for (int j = 0; j < NG; j++) {
            // a sum of 37 products through each of the three entry points, with both kinds of finish (lh5_finish; accp_reduce + nu as acc5_finish does)
            LH5 a1, a2, a4;
            lh5_zero(a1); lh5_zero(a2); lh5_zero(a4);
            AccP col[5];
            for (int q = 0; q < 5; q++) accp_zero(col[q]);
            R3 want = {{0, 0, 0}};
            R3 xs[40], ys[40];
            for (int k = 0; k < 40; k++) { triple((i + k) % NG, k % 3, xs[k], 1, 2); triple((j + 3 * k) % NG, (k + 1) % 3, ys[k], 5, 7); }
            for (int k = 0; k < 37; k++) {
                want = radd3(want, rmul3(xs[k], ys[k], NU40));
                lh5_mac(a1, f3(xs[k]), f3(ys[k]));
                const u64 *x = xs[k].c, *y = ys[k].c;
                accp_mad(col[0], x[0], y[0]);
                accp_mad(col[1], x[0], y[1]); accp_mad(col[1], x[1], y[0]);
                accp_mad(col[2], x[0], y[2]); accp_mad(col[2], x[1], y[1]); accp_mad(col[2], x[2], y[0]);
                accp_mad(col[3], x[1], y[2]); accp_mad(col[3], x[2], y[1]);
                accp_mad(col[4], x[2], y[2]);
            }
            for (int k = 0; k + 1 < 37; k += 2) lh5_mac2(a2, f3(xs[k]), f3(ys[k]), f3(xs[k + 1]), f3(ys[k + 1]));
            lh5_mac(a2, f3(xs[36]), f3(ys[36]));
            for (int k = 0; k + 3 < 37; k += 4) {
                Fq3 xa[4], ya[4];
                for (int q = 0; q < 4; q++) { xa[q] = f3(xs[k + q]); ya[q] = f3(ys[k + q]); }
                lh5_macn<4>(a4, xa, ya);
            }
            lh5_mac(a4, f3(xs[36]), f3(ys[36]));
            bad += !same(lh5_finish(a1), want) + !same(lh5_finish(a2), want) + !same(lh5_finish(a4), want);
            R3 viacol;
            viacol.c[0] = radd(accp_reduce(col[0]), rmul(NU40, accp_reduce(col[3])));
            viacol.c[1] = radd(accp_reduce(col[1]), rmul(NU40, accp_reduce(col[4])));
            viacol.c[2] = accp_reduce(col[2]);
            bad += !same(f3(viacol), want);
            Fq3 fast = fq3_from_columns_2p40(col);      // (37 products per column: still inside fq_from_lin's range)
            bad += !same(fast, want);
            n += 5;
        }
    group("lh5_mac lh5_mac2 lh5_macn<4> lh5_finish (37 terms)", n, bad);
}

// Largest number of products one thread adds into one LH5 / Acc5 accumulator before it is reduced:
//   k_dot_batch (lf_kernels.hip, launch_dot_batch: "if (gb > LF_DOT_BLOCKS) gb = LF_DOT_BLOCKS") strides 64 x 256 threads over a table of n <= m = 2^s entries,
//   s <= LF_S_MAX = 30 (lf_ccs_load, lf_capi.cpp: "p->s > LF_S_MAX") -> 2^30 / 2^14 = 65536 products; k_dot_eq (Acc5, RED_BLOCKS = 256) 16384;
//   the wide linearization rounds (lf_lin_wide.hip, LW_BLOCKS = 128) 2^29 pairs / 2^15 = 16384 per point; the fold rounds (lf_rounds.hip) start a fresh
//   accumulator per pair and add at most 2K * 3 = 192 tables; k_lincomb_z adds one term per table (at most 2K * t = 512).
// The two limits are constants of lf_field.cuh that the launch and the parameter check themselves use, so this count moves with them.
static const unsigned long long N_MAX = LF_LAZY_N_MAX;

static void test_lazy_long() {
    // the pair whose column sums have the largest |L| + |H|.  Only triples (x, x, x), (y, y, y) are searched: the middle column then is three times one F_p
    // product x y, the most a column of one F_{p^3} product holds.  That this is the worst case is not taken from the search: accp_lh bounds |H| by four 32-bit
    // pieces (< 2^34) for ANY column, and the |H| found here, 2^34.0, reaches that bound.
    int64_t best_l = 0, best_h = 0;
    u64 bx = 0, by = 0;
    for (int i = 0; i < NG; i++)
        for (int j = 0; j < NG; j++) {
            LH5 t; lh5_zero(t);
            lh5_mac(t, fq3_make(GRID[i], GRID[i], GRID[i]), fq3_make(GRID[j], GRID[j], GRID[j]));
            for (int q = 0; q < 5; q++) {
                const int64_t l = t.c[q].l < 0 ? -t.c[q].l : t.c[q].l, h = t.c[q].h < 0 ? -t.c[q].h : t.c[q].h;
                if (l + h > best_l + best_h) { best_l = l; best_h = h; bx = GRID[i]; by = GRID[j]; }
            }
        }
    printf("  grid:");
    for (int i = 0; i < NG; i++) printf(" %llx", (unsigned long long)GRID[i]);
    printf("\n  per-thread product maximum N_MAX = %llu (k_dot_batch: 2^%u entries over %u x 256 threads, lf_kernels.hip launch_dot_batch / lf_capi.cpp lf_ccs_load)\n", N_MAX,
           LF_S_MAX, LF_DOT_BLOCKS);
    printf("  largest column of one product on the grid: |L| = %lld, |H| = %lld at x = 0x%llx, y = 0x%llx\n", (long long)best_l, (long long)best_h,
           (unsigned long long)bx, (unsigned long long)by);
    // lh5_finish shifts H by 8 bits as a 64-bit integer: the sums must stay below 2^55
    const unsigned long long room = (unsigned long long)(((i128)1 << 55) / (best_h ? best_h : 1));
    printf("  H << 8 in lh5_finish holds up to %llu such products (%.1f x N_MAX)\n", room, (double)room / (double)N_MAX);
    unsigned long long n = 0, bad = 0;
    const R3 ops[2][2] = {{{{P - 1, P - 1, P - 1}}, {{P - 1, P - 1, P - 1}}}, {{{bx, bx, bx}}, {{by, by, by}}}};
    for (int o = 0; o < 2; o++) {
        const R3 pr = rmul3(ops[o][0], ops[o][1], NU40);
        LH5 a1, a2; lh5_zero(a1); lh5_zero(a2);
        AccP col[5];
        for (int q = 0; q < 5; q++) accp_zero(col[q]);
        const Fq3 x = f3(ops[o][0]), y = f3(ops[o][1]);
        for (unsigned long long k = 1; k <= N_MAX; k++) {
            lh5_mac(a1, x, y);
            if (!(k & 1)) lh5_mac2(a2, x, y, x, y);
            accp_mad(col[0], x.c[0], y.c[0]);
            accp_mad(col[1], x.c[0], y.c[1]); accp_mad(col[1], x.c[1], y.c[0]);
            accp_mad(col[2], x.c[0], y.c[2]); accp_mad(col[2], x.c[1], y.c[1]); accp_mad(col[2], x.c[2], y.c[0]);
            accp_mad(col[3], x.c[1], y.c[2]); accp_mad(col[3], x.c[2], y.c[1]);
            accp_mad(col[4], x.c[2], y.c[2]);
            if ((k & (k - 1)) == 0 || k == 37 || k == N_MAX - 1) {      // every power of two up to N_MAX
                const R3 want = rscale3(pr, k);
                bad += !same(lh5_finish(a1), want);
                if (!(k & 1)) bad += !same(lh5_finish(a2), want);
                R3 viacol;
                viacol.c[0] = radd(accp_reduce(col[0]), rmul(NU40, accp_reduce(col[3])));
                viacol.c[1] = radd(accp_reduce(col[1]), rmul(NU40, accp_reduce(col[4])));
                viacol.c[2] = accp_reduce(col[2]);
                bad += !same(f3(viacol), want);
                n += 3;
            }
        }
    }
    group("lazy sums of N <= N_MAX worst-case products", n, bad);
}

int main() {
    test_fp();
    test_acc();
    test_fq3();
    test_lh5();
    test_lazy_long();
    if (fails) { printf("%d group(s) failed\n", fails); return 1; }
    printf("selftest ok\n");
    return 0;
}
