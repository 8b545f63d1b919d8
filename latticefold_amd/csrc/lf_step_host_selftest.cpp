// lf_step_host_selftest.cpp -- the numeric host work of the sumcheck rounds (lf_step_host.h: eq weights, the 81-entry digit look-up table, the completion of a
// split round message and its invertibility test) against the definitions, for both rings, under the address and undefined-behaviour sanitizers.  A stand-alone
// program (make step-host-selftest): host code only, the host rings come from the ordinary library, no GPU.
#include <stdio.h>

#include "bb_host.h"
#include "lf_host.h"
#include "lf_step_host.h"

typedef uint64_t u64;
typedef uint32_t u32;

static u64 g_seed = 0x5eed0f01d5ULL;   // fixed: the same operands on every run
static u64 rnd() {                     // splitmix64
    u64 z = (g_seed += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static long g_bad = 0;

template <class V>
struct Check {
    typedef typename V::Ext Ext;
    const V &v;
    const char *ring;
    long n = 0;
    Ext zero() const { return V::ext_from_u64(0); }
    Ext one() const { return V::ext_from_u64(1); }
    Ext rand_ext() const {
        Ext r;
        for (int i = 0; i < V::TAU; i++) r.c[i] = rnd() % V::modulus();
        return r;
    }
    Ext rand_nonzero() const {
        for (;;) {
            Ext r = rand_ext();
            if (!lfs::ext_is_zero<V>(r)) return r;
        }
    }
    Ext small(int64_t k) const { return k >= 0 ? V::ext_from_u64((u64)k) : V::ext_sub(zero(), V::ext_from_u64((u64)-k)); }
    bool same(const Ext &a, const Ext &b) const { return memcmp(a.c, b.c, sizeof(a.c)) == 0; }
    void expect(bool ok, const char *what, int i, int j) {
        n++;
        if (!ok) { g_bad++; printf("MISMATCH %s: %s [%d][%d]\n", ring, what, i, j); }
    }
    void done(const char *what) { printf("%s %s: %ld checks ok\n", ring, what, n); n = 0; }
    // sum_e co[e] X^e by plain extension products
    Ext poly_at(const Ext *co, u32 deg, u32 X) const {
        Ext r = zero(), xp = one();
        for (u32 e = 0; e <= deg; e++) { r = V::ext_add(r, v.ext_mul(co[e], xp)); xp = v.ext_mul(xp, small(X)); }
        return r;
    }
    Ext eq_at(const Ext &b, u32 X) const { return V::ext_add(v.ext_mul(V::ext_sub(one(), b), small(1 - (int64_t)X)), v.ext_mul(b, small(X))); }
    // a message of degree <= deg (values at 0..deg, slot `slot` of prev) whose interpolation at x is `target`: nodes 1..deg random, node 0 solved for
    void prev_message(u32 deg, const Ext &x, const Ext &target, u32 slot, u64 *prev) const {
        Ext w[9], rest = zero();
        for (u32 j = 0; j <= deg; j++) {
            Ext num = one(), den = one();
            for (u32 k = 0; k <= deg; k++)
                if (k != j) { num = v.ext_mul(num, V::ext_sub(x, small(k))); den = v.ext_mul(den, small((int64_t)j - (int64_t)k)); }
            w[j] = v.ext_mul(num, v.ext_inv(den));
        }
        for (u32 j = 1; j <= deg; j++) {
            const Ext pj = rand_ext();
            memcpy(prev + (size_t)j * V::RE + V::TAU * slot, pj.c, sizeof(pj.c));
            rest = V::ext_add(rest, v.ext_mul(w[j], pj));
        }
        const Ext p0 = v.ext_mul(V::ext_sub(target, rest), v.ext_inv(w[0]));
        memcpy(prev + (size_t)0 * V::RE + V::TAU * slot, p0.c, sizeof(p0.c));
    }
    void put(u64 *buf, u32 X, u32 slot, const Ext &e) const { memcpy(buf + (size_t)X * V::RE + V::TAU * slot, e.c, sizeof(e.c)); }

    void fold_completion() {
        for (int rep = 0; rep < 8; rep++) {
            const Ext c = rand_nonzero(), bi = rand_nonzero(), x = rand_ext();
            std::vector<u64> A((size_t)3 * V::RE), G((size_t)5 * V::RE), prev((size_t)5 * V::RE), out((size_t)5 * V::RE, ~0ull);
            Ext want[8][5];
            for (u32 slot = 0; slot < 8; slot++) {
                const Ext Ac[4] = {rand_ext(), rand_ext(), rand_ext(), rand_ext()}, Gc[3] = {rand_ext(), rand_ext(), rand_ext()};
                for (u32 X = 0; X <= 4; X++) {
                    want[slot][X] = V::ext_add(v.ext_mul(v.ext_mul(c, eq_at(bi, X)), poly_at(Ac, 3, X)), poly_at(Gc, 2, X));
                    put(G.data(), X, slot, poly_at(Gc, 2, X));
                }
                for (u32 e = 0; e < 3; e++) put(A.data(), e, slot, Ac[e]);
                prev_message(4, x, V::ext_add(want[slot][0], want[slot][1]), slot, prev.data());
            }
            const lfs::SplitCoef<V> s = lfs::split_coef(v, c, bi);
            expect(s.ok, "split_coef on non-zero c, beta", rep, 0);
            lfs::complete_fold_split(v, s, A.data(), G.data(), prev.data(), x, out.data());
            for (u32 slot = 0; slot < 8; slot++)
                for (u32 X = 0; X <= 4; X++) expect(same(lfs::ext_load<V>(&out[(size_t)X * V::RE + V::TAU * slot]), want[slot][X]), "fold completion", slot, X);
        }
        done("fold completion (degree 4)");
    }
    void lin_completion() {
        for (u32 dT = 1; dT <= 7; dT++)
            for (int first = 0; first < 2; first++) {   // first: round 1, every T(X) evaluated and no previous message
                const u32 deg = dT + 1;
                const Ext c = first ? one() : rand_nonzero(), bi = rand_nonzero(), x = rand_ext();
                std::vector<u64> Tv((size_t)(dT + 1) * V::RE), prev((size_t)(deg + 1) * V::RE), out((size_t)(deg + 1) * V::RE, ~0ull);
                Ext want[8][9];
                for (u32 slot = 0; slot < 8; slot++) {
                    Ext Tc[8];
                    for (u32 e = 0; e <= dT; e++) Tc[e] = rand_ext();
                    for (u32 X = 0; X <= deg; X++) want[slot][X] = v.ext_mul(v.ext_mul(c, eq_at(bi, X)), poly_at(Tc, dT, X));
                    for (u32 X = 0; X <= dT; X++) put(Tv.data(), X, slot, (X == 1 && !first) ? rand_ext() : poly_at(Tc, dT, X));   // (X = 1 is not read)
                    prev_message(deg, x, V::ext_add(want[slot][0], want[slot][1]), slot, prev.data());
                }
                const lfs::SplitCoef<V> s = lfs::split_coef(v, c, bi);
                lfs::complete_lin_split(v, s, dT, Tv.data(), first ? nullptr : prev.data(), x, out.data());
                for (u32 slot = 0; slot < 8; slot++)
                    for (u32 X = 0; X <= deg; X++) expect(same(lfs::ext_load<V>(&out[(size_t)X * V::RE + V::TAU * slot]), want[slot][X]), "lin completion", (int)dT, (int)X);
            }
        done("linearization completion (dT 1..7)");
    }
    void invertibility() {
        const Ext c = rand_nonzero(), bi = rand_nonzero();
        expect(!lfs::split_coef(v, zero(), bi).ok, "zero c must not split", 0, 0);
        expect(!lfs::split_coef(v, c, zero()).ok, "zero beta must not split", 0, 1);
        const lfs::SplitCoef<V> s = lfs::split_coef(v, c, bi);
        expect(s.ok && same(v.ext_mul(s.c, s.cinv), one()) && same(v.ext_mul(s.bi, s.binv), one()), "inverses", 0, 2);
        done("invertibility test");
    }
    void weights() {
        for (u32 nbits = 0; nbits <= 3; nbits++) {
            Ext pt[3] = {rand_ext(), rand_ext(), rand_ext()}, W[8];
            lfs::eq_weights(v, pt, nbits, W);
            for (u32 b = 0; b < (1u << nbits); b++) {
                Ext w = one();
                for (u32 j = 0; j < nbits; j++) w = v.ext_mul(w, ((b >> j) & 1) ? pt[j] : V::ext_sub(one(), pt[j]));
                expect(same(W[b], w), "eq_weights", (int)nbits, (int)b);
            }
        }
        // c_round against the product of its factors
        Ext beta[4] = {rand_ext(), rand_ext(), rand_ext(), rand_ext()}, pt[4] = {rand_ext(), rand_ext(), rand_ext(), rand_ext()}, acc = one();
        for (u32 round = 1; round <= 5; round++) {
            expect(same(lfs::eq_prefix(v, beta, pt, round), acc), "eq_prefix", (int)round, 0);
            if (round <= 4) acc = v.ext_mul(acc, V::ext_add(v.ext_mul(V::ext_sub(one(), beta[round - 1]), V::ext_sub(one(), pt[round - 1])), v.ext_mul(beta[round - 1], pt[round - 1])));
        }
        done("eq_weights / eq_prefix");
    }
    void lut() {
        const Ext r1 = rand_ext(), r2 = rand_ext(), o1 = V::ext_sub(one(), r1), o2 = V::ext_sub(one(), r2);
        const Ext W[4] = {v.ext_mul(o1, o2), v.ext_mul(r1, o2), v.ext_mul(o1, r2), v.ext_mul(r1, r2)};
        std::vector<Ext> out(162);
        lfs::fold_lut81(v, r1, r2, out.data());
        for (int code = 0; code < 81; code++) {
            Ext want = zero();
            int cc = code;
            for (int b = 0; b < 4; b++, cc /= 3) want = V::ext_add(want, v.ext_mul(small(cc % 3 - 1), W[b]));
            expect(same(out[code], want), "fold_lut81 value", code, 0);
            expect(same(out[81 + code], v.ext_mul(want, want)), "fold_lut81 square", code, 1);
        }
        done("fold_lut81");
    }
    void all() { fold_completion(); lin_completion(); invertibility(); weights(); lut(); }
};

int main() {
    lf::HostRing gold;
    {
        u64 nonres, y[24];
        lf::default_ring(&nonres, y);
        if (lf::build_crt_tables(nonres, y, gold.T) != 0) { printf("MISMATCH goldilocks tables\n"); return 1; }
    }
    static lfbb::BbHostRing bb;
    {
        u64 nonres, y[8 * lfbb::TAU];
        lfbb::bb_default_ring(&nonres, y);
        if (lfbb::bb_build_tables(nonres, y, bb.T) != 0) { printf("MISMATCH babybear tables\n"); return 1; }
    }
    const lf::GoldV gv{gold};
    const lfbb::BbV bv{bb};
    Check<lf::GoldV>{gv, "goldilocks"}.all();
    Check<lfbb::BbV>{bv, "babybear"}.all();
    if (g_bad) { printf("step host selftest FAILED: %ld mismatches\n", g_bad); return 1; }
    printf("step host selftest ok\n");
    return 0;
}
