// bb_field_selftest.cpp -- the HOST side of bb_field.cuh against plain `%` on 64- and 128-bit integers, as a stand-alone program for a sanitizer build
// (`make bb-field-selftest`).  The BabyBear backend stores a residue as the centred Montgomery word x~ = centre(x 2^32 mod p) in [-H, H], and every bound of
// the header (nine products in one signed 64-bit column, the pre-centring of mred's high half, the doubling of the nu = 2 path) is a bound on that word: the
// operands here are the 30 DEVICE WORDS of the grid below (tests/field_corners.py: EDGE_BW) and the saturating pairs, whose column k is nine terms of +-H^2.
// The undefined-behaviour sanitizer turns a signed overflow in `2 * b`, `2 * off + diag`, `thi - q` or `a +- b` into a failure.
// No GPU is needed.  Prints one line per group and "selftest ok"; exit status 0 only when every group agreed.
#include <cstdio>
#include <cstdlib>
#include "bb_field.cuh"

using namespace lfbb;
typedef __int128 i128;
static const i64 P = 2013265921;
static const int32_t H = 0x3C000000;

// ---- the reference: canonical residues with %, nothing from bb_field.cuh ----
static i64 md(i128 v) { i64 r = (i64)(v % (i128)P); return r < 0 ? r + P : r; }
static i64 rpow(i64 a, i64 e) { i64 r = 1; a = md(a); while (e) { if (e & 1) r = md((i128)r * a); a = md((i128)a * a); e >>= 1; } return r; }
static const i64 R = md((i128)1 << 32), RINV = rpow(R, P - 2);
static i64 canon_of(i64 w) { return md((i128)w * RINV); }                       // device word -> canonical residue
static int32_t word_of(i64 x) { i64 w = md((i128)md(x) * R); return (int32_t)(w > H ? w - P : w); }   // canonical residue -> device word
static int32_t cen(i128 v) { i64 r = md(v); return (int32_t)(r > H ? r - P : r); }   // any integer -> its centred representative
struct R9 { i64 c[9]; };
static R9 rmul9(const R9 &a, const R9 &b, i64 nu) {
    i64 col[17];
    for (int k = 0; k < 17; k++) col[k] = 0;
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) col[i + j] = md((i128)col[i + j] + (i128)a.c[i] * b.c[j]);
    R9 r;
    for (int k = 0; k < 9; k++) r.c[k] = k + 9 < 17 ? md((i128)col[k] + (i128)nu * col[k + 9]) : col[k];
    return r;
}

static const int R32 = 268435454;             // 2^32 mod p
static const int NG = 30;
static const int32_t GRID[NG] = {0, 1, -1, 2, -2, H, -H, H - 1, -(H - 1), H / 2, -(H / 2), H / 2 + 1, -(H / 2 + 1), R32, -R32, 1 << 29, -(1 << 29),
                                 0x3B7F7F7F, -0x3B7F7F7F, 0x3B808080, -0x3B808080, 0x007F7F7F, -0x00808080, 0x7F, -0x80, 0x80, -0x81, 0x7FFF, 0x8000, -0x8000};

static int fails = 0;
static void group(const char *name, unsigned long long checks, unsigned long long bad) {
    printf("%-60s %10llu checks %s\n", name, checks, bad ? "MISMATCH" : "ok");
    if (bad) { printf("  %llu mismatching words\n", bad); fails++; }
}
static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u64 rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void test_fp() {
    unsigned long long n = 0, bad = 0;
    for (int i = 0; i < NG; i++) {
        const fe a = GRID[i];
        bad += centre(a) != a; n++;
        bad += centre(2 * a) != cen(2 * (i128)a); n++;
        bad += to_canon(a) != (u32)canon_of(a); n++;
        bad += from_canon((u64)canon_of(a)) != a; n++;
        bad += from_canon((u64)canon_of(a) + (u64)P) != a; n++;                    // (from_canon reduces its argument)
        bad += from_small(a) != word_of(a); n++;
        bad += from_int((i64)a) != word_of(a); n++;
        bad += from_int((i64)a * 0x100000001LL) != word_of(md((i128)a * 0x100000001LL)); n++;
        bad += fneg(a) != cen(-(i128)a); n++;
        for (int j = 0; j < NG; j++) {
            const fe b = GRID[j];
            bad += fadd(a, b) != cen((i128)a + b);
            bad += fsub(a, b) != cen((i128)a - b);
            bad += centre(a + b) != cen((i128)a + b);
            bad += fmul(a, b) != cen((i128)a * b % P * RINV);
            bad += mred((i64)a * (i64)b) != cen((i128)a * b % P * RINV);
            bad += to_canon(fmul(a, b)) != (u32)md((i128)canon_of(a) * canon_of(b));
            bad += fmul_small(a, b) != cen((i128)a * b);
            n += 7;
        }
    }
    group("centre fadd fsub fneg fmul mred to_canon from_canon from_small", n, bad);
    n = bad = 0;
    const i64 col = 9 * (i64)H * H;                                                    // the whole range of mred's argument: its ends, steps around the
    const i64 ts[] = {col, -col, col - 1, 1 - col, (i64)H << 32, -((i64)H << 32), ((i64)H << 32) + 1, (((i64)H + 1) << 32) - 1, ((i64)H + 1) << 32,   // pre-centring
                      -(((i64)H + 1) << 32), -(((i64)H + 1) << 32) - 1, -(((i64)H) << 32) - 1, 0x7FFFFFFFLL << 32, 0xFFFFFFFFLL, 0x100000000LL, -1, -0x100000000LL, 0};
    for (i64 T : ts) if (T <= col && T >= -col) { bad += mred(T) != cen((i128)T % P * RINV); n++; }
    for (int k = 0; k < 200000; k++) {
        const i64 T = (i64)((i128)(rng() % (2 * (u64)col + 1)) - col);
        bad += mred(T) != cen((i128)T % P * RINV); n++;
    }
    const int32_t smalls[] = {0x7FFFFFFF, -0x7FFFFFFF, 0x40000000, -0x40000000, 0x7FFFFFFE};
    for (int32_t s : smalls) { bad += from_small(s) != word_of(s); n++; }
    const i64 ints[] = {INT64_MAX, -INT64_MAX, INT64_MIN, P, -P, P - 1, 1 - P, (i64)1 << 62, -((i64)1 << 62)};
    for (i64 s : ints) { bad += from_int(s) != word_of(md((i128)s)); n++; }
    group("mred over [-9H^2, 9H^2], from_small, from_int at their ends", n, bad);
}

static E9 e9w(const int32_t *w) { E9 r; for (int i = 0; i < 9; i++) r.c[i] = w[i]; return r; }
static R9 r9(const E9 &a) { R9 r; for (int i = 0; i < 9; i++) r.c[i] = canon_of(a.c[i]); return r; }
static bool same(const E9 &a, const R9 &b) { for (int i = 0; i < 9; i++) if (a.c[i] != word_of(b.c[i])) return false; return true; }
static i64 generic_nu() {                     // a primitive 24th root of unity (the other ring of the GPU tests); any constant would do for the arithmetic
    for (i64 g = 2;; g++) {
        const i64 z = rpow(g, (P - 1) / 24);
        if (rpow(z, 12) != 1 && rpow(z, 8) != 1) return z;
    }
}
static unsigned long long top_cols = 0, pre_cols = 0;
static double top_seen = 0;

static void test_e9() {
    unsigned long long n = 0, bad = 0;
    const i64 nug = generic_nu();
    const fe nugw = word_of(nug);
    auto one = [&](const E9 &a, const E9 &b) {
        const R9 ra = r9(a), rb = r9(b);
        const E9 b2 = e9_times_nu_t<true>(b, BB_TWO), b2g = e9_times_nu_t<false>(b, BB_TWO), bg = e9_times_nu_t<false>(b, nugw);
        for (int i = 0; i < 9; i++) {
            bad += b2.c[i] != cen(2 * (i128)b.c[i]) || b2g.c[i] != b2.c[i] || bg.c[i] != word_of(md((i128)rb.c[i] * nug));
            n++;
        }
        const R9 want2 = rmul9(ra, rb, 2), wantg = rmul9(ra, rb, nug);
        bad += !same(e9_mul_pre(a, b, b2), want2) + !same(e9_mul_pre(a, b, bg), wantg) + !same(e9_mul(a, b, BB_TWO), want2) + !same(e9_mul_t<true>(a, b, BB_TWO), want2);
        bad += !same(e9_sqr_pre(b, b2), rmul9(rb, rb, 2)) + !same(e9_sqr_pre(b, bg), rmul9(rb, rb, nug)) + !same(e9_sqr_pre(a, e9_times_nu_t<true>(a, BB_TWO)), rmul9(ra, ra, 2));
        n += 7;
        i64 T[9];
        e9_mul_cols(a, b, b2, T);
        for (int k = 0; k < 9; k++) {
            i128 t = 0;
            for (int i = 0; i < 9; i++) t += (i128)a.c[i] * (i <= k ? b.c[k - i] : b2.c[k + 9 - i]);
            const i128 lim = 9 * (i128)H * H;
            bad += t != (i128)T[k] || t > lim || t < -lim || mred(T[k]) != word_of(want2.c[k]);
            const double f = (double)(T[k] < 0 ? -T[k] : T[k]) / 9223372036854775808.0;
            if (f > top_seen) top_seen = f;
            top_cols += f > 0.9;
            pre_cols += (T[k] >> 32) > H || (T[k] >> 32) < -H;
            n++;
        }
        const int32_t scal[] = {0, 1, -1, 3, -128, 127, 0x7FFFFFFF, -0x7FFFFFFF};
        for (int32_t s : scal) {
            const E9 m = e9_mul_small(a, s);
            for (int i = 0; i < 9; i++) bad += m.c[i] != cen((i128)a.c[i] * s);
            n++;
        }
        bad += !e9_eq(e9_add(a, b), e9_add(b, a)) + !same(e9_add(a, b), [&] { R9 r; for (int i = 0; i < 9; i++) r.c[i] = md((i128)ra.c[i] + rb.c[i]); return r; }());
        bad += !same(e9_sub(a, b), [&] { R9 r; for (int i = 0; i < 9; i++) r.c[i] = md((i128)ra.c[i] - rb.c[i]); return r; }());
        n += 3;
    };
    // the saturating pairs of nu = 2 and of the generic nu: a_i = +-H, b_j = H (j <= k), nu b_j = H (j > k)
    const fe halfg = word_of(md((i128)canon_of(H) * rpow(nug, P - 2)));
    for (int sign = 1; sign >= -1; sign -= 2)
        for (int k = 0; k < 9; k++)
            for (int gen = 0; gen < 2; gen++) {
                int32_t aw[9], bw[9];
                for (int j = 0; j < 9; j++) { aw[j] = sign * H; bw[j] = j <= k ? H : gen ? halfg : H / 2; }
                one(e9w(aw), e9w(bw));
                for (int j = 0; j < 9; j++) bw[j] = -bw[j];
                one(e9w(aw), e9w(bw));
            }
    // every pair of grid words in every pair of coordinate positions (tests/field_corners.py: all_pairs), then grid elements drawn at random
    for (int sh = 0; sh < 9; sh++)
        for (int x = 0; x < NG; x++)
            for (int y = 0; y < NG; y++) {
                int32_t aw[9], bw[9];
                for (int q = 0; q < 9; q++) { aw[q] = GRID[(x + q * sh) % NG]; bw[q] = GRID[(y + 5 * q * sh) % NG]; }
                one(e9w(aw), e9w(bw));
            }
    for (int k = 0; k < 20000; k++) {
        int32_t aw[9], bw[9];
        for (int q = 0; q < 9; q++) { aw[q] = GRID[rng() % NG]; bw[q] = GRID[rng() % NG]; }
        one(e9w(aw), e9w(bw));
    }
    printf("  largest column: %.5f * 2^63; columns above 0.9 * 2^63: %llu; columns whose high half mred centres first: %llu\n", top_seen, top_cols, pre_cols);
    if (top_seen < 0.98 || !top_cols || !pre_cols) { printf("  the operands do not reach the top of the column\n"); fails++; }
    group("e9_times_nu_t e9_mul_pre e9_sqr_pre e9_mul_cols e9_mul_small", n, bad);
}

int main() {
    printf("  grid:");
    for (int i = 0; i < NG; i++) printf(" %d", GRID[i]);
    printf("\n");
    test_fp();
    test_e9();
    if (fails) { printf("%d group(s) failed\n", fails); return 1; }
    printf("selftest ok\n");
    return 0;
}
