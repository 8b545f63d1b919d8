// lf_field_selftest_a3p.cpp -- the three-column lazy sums of lf_field.cuh (A3P, its folded form LH3, fq3_premul_2p40, fq3_mul_2p40_pre) on the HOST against `unsigned __int128 %`,
// as a stand-alone program for a sanitizer build (`make field-selftest-a3p`).  Reference arithmetic below uses nothing from the header; residues are added in
// 128 bits (two residues below p do not fit 64).  Checked: corner and random operands, sums of 1, 2, 37, 288 and 3 * 65 536 products, the all-(p-1) and
// all-(2^64-1) sums (every counter of every column non-zero), equality with lh5_mac + lh5_finish and with fq3_mul_2p40, and the reduced product with a
// pre-multiplied operand.  No GPU is needed.  Prints one line per group and "a3p selftest ok"; exit status 0 only when every group agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lf_field.cuh"

using namespace lf;
typedef unsigned __int128 u128;
static const u64 P = 0xFFFFFFFF00000001ULL;
static const u64 NU40 = 1ULL << 40;

// ---- the reference: plain 128-bit arithmetic and %, nothing from lf_field.cuh; operands may be ANY 64-bit words ----
static u64 radd(u64 a, u64 b) { return (u64)(((u128)(a % P) + (b % P)) % P); }
static u64 rmul(u64 a, u64 b) { return (u64)(((u128)(a % P) * (b % P)) % P); }
struct R3 { u64 c[3]; };
static R3 rmul3(const R3 &a, const R3 &b) {
    u64 col[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) col[i + j] = radd(col[i + j], rmul(a.c[i], b.c[j]));
    R3 r;
    r.c[0] = radd(col[0], rmul(NU40, col[3]));
    r.c[1] = radd(col[1], rmul(NU40, col[4]));
    r.c[2] = col[2];
    return r;
}
static R3 radd3(const R3 &a, const R3 &b) { R3 r; for (int i = 0; i < 3; i++) r.c[i] = radd(a.c[i], b.c[i]); return r; }
static R3 rscale3(const R3 &a, u64 k) { R3 r; for (int i = 0; i < 3; i++) r.c[i] = rmul(a.c[i], k); return r; }

// the corner operands: 0, 1, p-1, p, 2^64-1, 2^32-1, 2^32, p-2^24 (p and 2^64-1 are loose words: the lazy forms take them, the canonical-input ones do not)
static const u64 CORN[8] = {0, 1, P - 1, P, ~0ULL, 0xFFFFFFFFULL, 1ULL << 32, P - (1ULL << 24)};
static const int NC = 8, NCANON = 6;
static const u64 CANON[NCANON] = {0, 1, P - 1, 0xFFFFFFFFULL, 1ULL << 32, P - (1ULL << 24)};

static int fails = 0;
static void group(const char *name, unsigned long long checks, unsigned long long bad) {
    printf("%-58s %10llu checks %s\n", name, checks, bad ? "MISMATCH" : "ok");
    if (bad) { printf("  %llu mismatches\n", bad); fails++; }
}
static Fq3 f3(const R3 &a) { return fq3_make(a.c[0], a.c[1], a.c[2]); }
static bool same(const Fq3 &a, const R3 &b) { return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2]; }
static u64 rng_state = 0xD1B54A32D192ED03ULL;
static u64 rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
// loose = true: any 64-bit word (corners included); false: canonical residues only (what lh5_mac / fq3_mul_2p40 are specified for)
static u64 word(bool loose) {
    const u64 r = rng();
    if (r & 1) return loose ? CORN[(r >> 8) % NC] : CANON[(r >> 8) % NCANON];
    const u64 w = rng();
    return loose ? w : w % P;
}
static R3 r3(bool loose) { R3 a; for (int q = 0; q < 3; q++) a.c[q] = word(loose); return a; }

static void test_premul() {
    unsigned long long n = 0, bad = 0;
    for (int i = 0; i < NC; i++) { bad += fq_mul_2p40_loose(CORN[i]) % P != rmul(CORN[i], NU40); n++; }
    for (int k = 0; k < 100000; k++) {
        const u64 w = rng();
        bad += fq_mul_2p40_loose(w) % P != rmul(w, NU40);
        bad += fq_mul_2p40_loose(w >> (k % 64)) % P != rmul(w >> (k % 64), NU40);
        n += 2;
    }
    group("fq_mul_2p40_loose (any 64-bit word)", n, bad);
}

// one sum of `len` products through every form.  canon: operands are residues, so lh5 and fq3_mul_2p40 apply too
static void one_sum(const std::vector<R3> &xs, const std::vector<R3> &ys, bool canon, bool with_lh5, unsigned long long &n, unsigned long long &bad) {
    const size_t len = xs.size();
    A3P acc; a3p_zero(acc);
    LH3 l3; lh3_zero(l3);
    LH5 lh; lh5_zero(lh);
    R3 want = {{0, 0, 0}}, viamul = {{0, 0, 0}};
    for (size_t k = 0; k < len; k++) {
        const Fq3 x = f3(xs[k]), y = f3(ys[k]);
        const Fq3Nu yn = fq3_premul_2p40(y);
        a3p_mac(acc, x, y, yn);
        lh3_mac(l3, x, y, yn);
        want = radd3(want, rmul3(xs[k], ys[k]));
        if (canon) {
            if (with_lh5) lh5_mac(lh, x, y);
            const Fq3 pr = fq3_mul_2p40(x, y);
            const R3 prr = {{pr.c[0], pr.c[1], pr.c[2]}};
            viamul = radd3(viamul, prr);
            if (k < 64 || k + 1 == len) {       // the reduced product with a pre-multiplied operand, both ways round
                const Fq3 p1 = fq3_mul_2p40_pre(x, y, yn), p2 = fq3_mul_2p40_pre(y, x, fq3_premul_2p40(x));
                bad += !fq3_eq(p1, pr) + !fq3_eq(p2, pr) + !same(pr, rmul3(xs[k], ys[k]));
                n += 3;
            }
        }
    }
    const Fq3 got = a3p_finish(acc);
    bad += !same(got, want); n++;
    bad += !same(lh3_finish(l3), want); n++;      // the folded three-column form: same words
    bad += got.c[0] >= P || got.c[1] >= P || got.c[2] >= P; n++;       // canonical
    if (canon) {
        bad += !same(got, viamul); n++;
        if (with_lh5) { bad += !fq3_eq(got, lh5_finish(lh)); n++; }
    }
}

static void test_sums() {
    const size_t lens[] = {1, 2, 37, 288};
    unsigned long long n = 0, bad = 0;
    // every corner pair in every coordinate position, as the first product of each length
    for (size_t len : lens)
        for (int canon = 0; canon < 2; canon++) {
            const u64 *g = canon ? CANON : CORN;
            const int ng = canon ? NCANON : NC;
            for (int i = 0; i < ng; i++)
                for (int j = 0; j < ng; j++)
                    for (int sh = 0; sh < 3; sh++) {
                        std::vector<R3> xs(len), ys(len);
                        for (size_t k = 0; k < len; k++) {
                            for (int q = 0; q < 3; q++) {
                                xs[k].c[q] = g[(i + (q + sh) * (int)(k + 1)) % ng];
                                ys[k].c[q] = g[(j + 3 * (q + 2 * sh) * (int)(k + 1) + (int)k) % ng];
                            }
                        }
                        one_sum(xs, ys, canon, true, n, bad);
                    }
        }
    group("a3p sums of 1, 2, 37, 288 corner products", n, bad);
    n = bad = 0;
    for (int it = 0; it < 4000; it++) {
        const size_t len = it < 1000 ? lens[it % 4] : 1 + rng() % 200;
        const bool canon = it & 1;
        std::vector<R3> xs(len), ys(len);
        for (size_t k = 0; k < len; k++) { xs[k] = r3(!canon); ys[k] = r3(!canon); }
        one_sum(xs, ys, canon, true, n, bad);
    }
    group("a3p sums of random / corner mixes (1..288 products)", n, bad);
}

static void test_long() {
    // 3 * 65 536 products (three times the longest per-thread sum of any launch): all p-1, all 2^64-1, and a random canonical run.  lh5 takes part up to its
    // own range only (65 536 worst-case products); beyond it the integers and the sum of fq3_mul_2p40 are the references.
    const unsigned long long N = 3ULL * LF_LAZY_N_MAX;
    unsigned long long n = 0, bad = 0;
    const u64 fills[2] = {P - 1, ~0ULL};
    for (int o = 0; o < 2; o++) {
        const R3 v = {{fills[o], fills[o], fills[o]}};
        const R3 pr = rmul3(v, v);
        const Fq3 x = f3(v);
        const Fq3Nu xn = fq3_premul_2p40(x);
        A3P acc; a3p_zero(acc);
        LH3 l3; lh3_zero(l3);
        LH5 lh; lh5_zero(lh);
        for (unsigned long long k = 1; k <= N; k++) {
            a3p_mac(acc, x, x, xn);
            lh3_mac(l3, x, x, xn);
            if (o == 0 && k <= LF_LAZY_N_MAX) lh5_mac(lh, x, x);
            if ((k & (k - 1)) == 0 || k == 37 || k == 288 || k == N) {
                bad += !same(a3p_finish(acc), rscale3(pr, k)); n++;
                bad += !same(lh3_finish(l3), rscale3(pr, k)); n++;
                if (o == 0 && k <= LF_LAZY_N_MAX) { bad += !fq3_eq(a3p_finish(acc), lh5_finish(lh)); n++; }
            }
            if (k == 2 && o == 1) {       // 2^64 - 1 has both halves full: from the second product on every counter of every column counts
                for (int q = 0; q < 3; q++) { bad += !(acc.c[q].c00 && acc.c[q].c01 && acc.c[q].c11); n++; }     // (p - 1 has a zero low half: its sums exercise c11)
            }
        }
        printf("  %llu x (0x%llx, .., ..)^2: column 0 counters c00 / c01 / c11 = %u / %u / %u\n", N, (unsigned long long)fills[o], acc.c[0].c00, acc.c[0].c01,
               acc.c[0].c11);
        for (int q = 0; q < 3; q++) { bad += acc.c[q].c01 > 6 * N || acc.c[q].c00 > 3 * N || acc.c[q].c11 > 3 * N; n++; }    // the range comment of lf_field.cuh
    }
    {
        std::vector<R3> xs(N), ys(N);
        for (unsigned long long k = 0; k < N; k++) { xs[k] = r3(false); ys[k] = r3(false); }
        one_sum(xs, ys, true, false, n, bad);
    }
    group("a3p sums of 3 x 65 536 products", n, bad);
}

static void test_pre() {
    unsigned long long n = 0, bad = 0;
    for (int i = 0; i < NCANON; i++)
        for (int j = 0; j < NCANON; j++)
            for (int sh = 0; sh < 9; sh++) {
                R3 a, b;
                for (int q = 0; q < 3; q++) { a.c[q] = CANON[(i + q * (sh % 3)) % NCANON]; b.c[q] = CANON[(j + q * (sh / 3) + 2 * q) % NCANON]; }
                const Fq3 want = fq3_mul_2p40(f3(a), f3(b));
                bad += !fq3_eq(fq3_mul_2p40_pre(f3(a), f3(b), fq3_premul_2p40(f3(b))), want) + !same(want, rmul3(a, b));
                n += 2;
            }
    for (int k = 0; k < 200000; k++) {
        const R3 a = r3(false), b = r3(false);
        const Fq3 want = fq3_mul_2p40(f3(a), f3(b)), got = fq3_mul_2p40_pre(f3(a), f3(b), fq3_premul_2p40(f3(b)));
        bad += !fq3_eq(got, want) + !same(got, rmul3(a, b));
        n += 2;
    }
    // a square through its own multiples (the round kernels' f0^2, df^2)
    for (int k = 0; k < 50000; k++) {
        const R3 a = r3(false);
        bad += !same(fq3_mul_2p40_pre(f3(a), f3(a), fq3_premul_2p40(f3(a))), rmul3(a, a)); n++;
    }
    group("fq3_mul_2p40_pre against fq3_mul_2p40 and the integers", n, bad);
}

int main() {
    test_premul();
    test_sums();
    test_long();
    test_pre();
    if (fails) { printf("%d group(s) failed\n", fails); return 1; }
    printf("a3p selftest ok\n");
    return 0;
}
