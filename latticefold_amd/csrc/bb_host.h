// bb_host.h -- host-side pieces of the BabyBearRingNTT backend: ring tables (data-driven CRT), ring operations on a
// handful of elements (canonical u64 words, plain % arithmetic: O(proof size) only), Poseidon + Fiat-Shamir transcript (sponge and table
// builders: poseidon_host.h).
// Reference anchors: cyclotomic-rings/src/rings/babybear.rs:1-68 (ring aliases, challenge set),
// rings/poseidon/babybear.rs:7-1425 (Poseidon parameters), latticefold/src/transcript/poseidon.rs:29-75.
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>

#include "bb_field.cuh"
#include "poseidon_host.h"

namespace lfbb {

struct H9 { u64 c[TAU]; };   // canonical F_{p^9} element on the host

// Tables for the structured CRT.  a(X) = sum_{r<9} X^r A_r(X^9); A_r is evaluated at the 8 primitive 24th roots by the
// same three radix-2 layers as the Goldilocks ring (U^8 - U^4 + 1), then X^r -> tw[r][p] * Y^pos[r][p] in slot_of_pos[p].
struct BbTables {
    u64 nu;                       // F_{p^9} = F_p[Y]/(Y^9 - nu), canonical
    H9 y[8];                      // image of X in slot k
    u64 w4, w2, w10, w1, w7, w5, w11;
    int slot_of_pos[8];
    int pos[TAU][8];              // pos[0][p] = 0
    u64 tw[TAU][8];               // tw[0][p] = 1
    H9 ypow[8][D];                // dense CRT: slot_k = sum_c a_c * ypow[k][c]
    u64 icrt[D][D];               // dense inverse
};
void bb_default_ring(u64 *nonres, u64 y[8 * TAU]);
int bb_build_tables(u64 nonres, const u64 *y, BbTables &out);   // 0 or <0

inline u64 hmul(u64 a, u64 b) { return a * b % BB_P; }
inline u64 hadd(u64 a, u64 b) { u64 r = a + b; return r >= BB_P ? r - BB_P : r; }
inline u64 hsub(u64 a, u64 b) { return a >= b ? a - b : a + BB_P - b; }
u64 hpow(u64 a, u64 e);
inline u64 hinv(u64 a) { return hpow(a, BB_P - 2); }
inline u64 hfrom_i64(int64_t v) { int64_t r = v % (int64_t)BB_P; return (u64)(r < 0 ? r + (int64_t)BB_P : r); }

// inverse in F_p[Y]/(Y^9 - nu): solve (multiplication by a) x = 1 by Gaussian elimination on the 9 x 9 matrix M[i][j] = [Y^i](a Y^j); false if a = 0
bool h9_inv(const H9 &a, u64 nu, H9 *out);
struct BbHostRing {
    BbTables T;
    H9 mul9(const H9 &a, const H9 &b) const;
    void crt(const u64 *coef, u64 *ntt) const;
    void icrt(const u64 *ntt, u64 *coef) const;
    void mul_ntt(const u64 *a, const u64 *b, u64 *out) const;
    void mul_h9(const u64 *a, const H9 &s, u64 *out) const;
    static void add(const u64 *a, const u64 *b, u64 *out);
    static void sub(const u64 *a, const u64 *b, u64 *out);
    static void from_u64(u64 v, u64 *out);
    static void from_h9(const H9 &s, u64 *out);
};
void bb_balanced_digits(u64 v, u64 base, unsigned digits, int64_t *out, int mode = 0);

struct BbField {   // field policy of poseidon_host.h
    static constexpr u64 P = BB_P;
    static u64 add(u64 a, u64 b) { return hadd(a, b); }
    static u64 sub(u64 a, u64 b) { return hsub(a, b); }
    static u64 mul(u64 a, u64 b) { return hmul(a, b); }
    static u64 inv(u64 a) { return hinv(a); }
    static u64 from_word(u64 x) { return x % BB_P; }
};
class BbTranscript {
  public:
    BbTranscript();
    void absorb_fq(const u64 *x, size_t n);
    void absorb_ring(const u64 *elems, size_t count);
    void absorb_label(const char *ascii);
    void absorb_h9_as_ring(const H9 &c);
    void absorb_u64_as_ring(u64 v);
    H9 get_challenge();                            // squeeze tau words, absorb them back
    void get_short_challenge(u64 coeff_out[D]);    // 18 bytes -> 24 coefficients in [-32,32), zero-padded to degree 72
    static void permute(u64 st[24]);               // sparse-factorised partial rounds; AVX2 Montgomery lanes when available
    static void permute_scalar(u64 st[24]);        // same factorisation, scalar (reference for the SIMD path)
    static void permute_plain(u64 st[24]);
    static void params(const u64 **ark, const u64 **mds);
    // external-basis hook, as lf::Transcript::set_basis (T, Ti: 9x9 row-major, ext = T int; nullptr = off)
    void set_basis(const u64 *T, const u64 *Ti) { bT_ = T; bTi_ = Ti; }

    void squeeze(u64 *out, size_t n);   // raw field elements of the sponge (lf_transcript_squeeze_bytes)

  private:
    poseidon::Sponge<BbField, &BbTranscript::permute> sp_;
    const u64 *bT_ = nullptr, *bTi_ = nullptr;
};

#pragma GCC visibility push(hidden)   // (not part of the ABI)
inline H9 h9_load(const u64 *w) { H9 r; for (int i = 0; i < TAU; i++) r.c[i] = w[i] % BB_P; return r; }
inline H9 h9_zero() { H9 r; memset(&r, 0, sizeof(r)); return r; }
inline H9 h9_one() { H9 r = h9_zero(); r.c[0] = 1; return r; }
inline H9 h9_sub(const H9 &a, const H9 &b) { H9 r; for (int i = 0; i < TAU; i++) r.c[i] = hsub(a.c[i], b.c[i]); return r; }
inline H9 h9_add(const H9 &a, const H9 &b) { H9 r; for (int i = 0; i < TAU; i++) r.c[i] = hadd(a.c[i], b.c[i]); return r; }
inline H9 h9_scale(const H9 &a, u64 k) { H9 r; for (int i = 0; i < TAU; i++) r.c[i] = hmul(a.c[i], k % BB_P); return r; }

// ---- host policy of lf_step_host.h / lf_verify.h on this ring: small inline functions over a host ring it REFERS to (a context's, or the default one) ------
struct BbV {
    static constexpr int RE = lfbb::RE, TAU = lfbb::TAU;
    static u64 modulus() { return BB_P; }
    typedef H9 Ext;
    typedef BbTranscript Tr;
    const BbHostRing &ring;
    void mul(const u64 *a, const u64 *b, u64 *o) const { ring.mul_ntt(a, b, o); }
    void mul_ext(const u64 *a, const Ext &s, u64 *o) const { ring.mul_h9(a, s, o); }
    static void add(const u64 *a, const u64 *b, u64 *o) { BbHostRing::add(a, b, o); }
    static void sub(const u64 *a, const u64 *b, u64 *o) { BbHostRing::sub(a, b, o); }
    static void from_u64(u64 v, u64 *o) { BbHostRing::from_u64(v, o); }
    static void from_ext(const Ext &e, u64 *o) { BbHostRing::from_h9(e, o); }
    static bool is_diag(const u64 *e, Ext *out) {
        for (int k = 1; k < 8; k++)
            if (memcmp(e + TAU * k, e, TAU * 8)) return false;
        if (out) *out = h9_load(e);
        return true;
    }
    static Ext ext_from_u64(u64 v) { Ext r = h9_zero(); r.c[0] = v % BB_P; return r; }
    Ext ext_mul(const Ext &a, const Ext &b) const { return ring.mul9(a, b); }
    static Ext ext_add(const Ext &a, const Ext &b) { return h9_add(a, b); }
    static Ext ext_sub(const Ext &a, const Ext &b) { return h9_sub(a, b); }
    Ext ext_inv(const Ext &a) const { Ext r; return h9_inv(a, ring.T.nu, &r) ? r : h9_zero(); }
    static Ext ext_scale(const Ext &a, u64 k) { return h9_scale(a, k); }   // times a base-field word
    static u64 finv(u64 a) { return hinv(a); }
    static void absorb_ext(Tr &tr, const Ext &e) { tr.absorb_h9_as_ring(e); }
    void crt(const u64 *c, u64 *o) const { ring.crt(c, o); }
    void icrt(const u64 *x, u64 *o) const { ring.icrt(x, o); }
    static u64 fmul(u64 a, u64 b) { return hmul(a % BB_P, b % BB_P); }
    static u64 fadd(u64 a, u64 b) { return hadd(a, b); }
    static u64 from_i64(int64_t v) { return hfrom_i64(v); }
    static void balanced_digits(u64 v, u64 base, unsigned digits, int64_t *out, int mode) { bb_balanced_digits(v, base, digits, out, mode); }
    // accumulation of the v_0 product (lfs::fold_v0): lazy.  The coefficients of a short challenge are small signed integers (|rho_a| <= 32) and theta words
    // are < 2^31, so the terms are plain signed 64-bit multiply-adds with ONE reduction per output word: a word of the degree-142 product collects at most
    // 32 * 72 terms of < 2^5 * 2^31, and the reduction by X^72 = X^36 - 1 adds at most two more words to each -- |acc| < 3 * 72 * 32 * 2^36 < 2^50.
    typedef int64_t Acc;
    static Acc acc_coef(u64 c) { c %= BB_P; return c > BB_P / 2 ? (int64_t)c - (int64_t)BB_P : (int64_t)c; }
    static void acc_mac(Acc *d, const u64 *t, int n, Acc r) { for (int x = 0; x < n; x++) d[x] += (int64_t)t[x] * r; }
    static void acc_fold(Acc &mid, Acc &lo, Acc top) { mid += top; lo -= top; }   // X^d = X^(d - RE/2) - X^(d - RE)
    static u64 acc_word(Acc a) { return hfrom_i64(a); }
};
#pragma GCC visibility pop

}  // namespace lfbb
