// lf_host.h -- host-side pieces of the MI355X LatticeFold prover: ring tables (data-driven CRT), small
// ring operations on a handful of elements, Poseidon/Grain, Fiat-Shamir transcript (sponge and table builders: poseidon_host.h).
// Everything bulk runs on the GPU (lf_kernels.hip); this file only handles O(proof size) data.
#pragma once
#include <stddef.h>
#include <string>
#include <vector>

#include "lf_field.cuh"
#include "poseidon_host.h"

namespace lf {

constexpr int D = 24;      // ring degree, Phi_72 = X^24 - X^12 + 1 (cyclotomic-rings/src/rings/goldilocks.rs:19)
constexpr int SLOTS = 8;   // NTT slots
constexpr int TAU = 3;     // extension degree of each slot
constexpr int RE = 24;     // u64 words per ring element

// Butterfly data for the structured CRT, derived from the (data) cube roots y_k; see lf_ring.cpp.
struct CrtTables {
    u64 nu;           // F_{p^3} non-residue
    int nu_is_2p40;   // fast path flag
    Fq3 y[8];         // image of X in slot k
    // forward butterflies relative to omega = y_0^3
    u64 w4, w2, w10, w1, w7, w5, w11;        // omega^4, omega^2, omega^10, omega, omega^7, omega^5, omega^11
    // inverse butterflies
    u64 inv_1m2w4;                            // 1/(1 - 2 omega^4)
    u64 i2w2, i2w10, i2w1, i2w7, i2w5, i2w11; // 1/(2 omega^e)
    u64 inv2;                                 // 1/2
    // natural butterfly position p -> slot, and per natural position the monomial twist
    int slot_of_pos[8];
    int pos1[8], pos2[8];    // F_{p^3} coordinate receiving A_1 / A_2
    u64 tw1[8], tw2[8];      // multipliers for A_1 / A_2
    u64 itw1[8], itw2[8];    // their inverses
    // dense form for the host (and the generic validation path): slot_k = sum_c a_c * ypow[k][c]
    Fq3 ypow[8][24];
    u64 icrt[24][24];
};

// default tables (NU = 2^40, ascending exponents; see DESIGN.md "CRT map is data")
void default_ring(u64 *nonres, u64 y[24]);
// returns 0 or <0 (LF_ERR_BAD_TABLES)
int build_crt_tables(u64 nonres, const u64 y[24], CrtTables &out);

// ---- host ring helpers on canonical AoS elements (24 words) ------------------------------------------------
struct HostRing {
    CrtTables T;
    Fq3 mul3(Fq3 a, Fq3 b) const { return T.nu_is_2p40 ? fq3_mul<true>(a, b, T.nu) : fq3_mul<false>(a, b, T.nu); }
    Fq3 inv3(Fq3 a) const { return T.nu_is_2p40 ? fq3_inv<true>(a, T.nu) : fq3_inv<false>(a, T.nu); }
    void crt(const u64 *coef, u64 *ntt) const;
    void icrt(const u64 *ntt, u64 *coef) const;
    void mul_ntt(const u64 *a, const u64 *b, u64 *out) const;      // slot-wise
    void mul_fq3(const u64 *a, Fq3 s, u64 *out) const;             // times diagonal embedding
    static void add(const u64 *a, const u64 *b, u64 *out);
    static void sub(const u64 *a, const u64 *b, u64 *out);
    static void from_u64(u64 v, u64 *out);                          // R::from(u128)
    static void from_fq3(Fq3 s, u64 *out);                          // R::from(BaseRing)
    static bool is_diag(const u64 *e, Fq3 *out);
};

// balanced digits of one canonical coefficient (stark_rings::balanced_decomposition)
void balanced_digits(u64 v, u64 base, unsigned digits, int64_t *out, int mode = 0);   // mode: see lf_set_digit_mode

// ---- Poseidon + transcript (crates/latticefold/src/transcript/poseidon.rs:29-75) ------------------------------
struct FqField {   // field policy of poseidon_host.h
    static constexpr u64 P = LF_P;
    static u64 add(u64 a, u64 b) { return fq_add(a, b); }
    static u64 sub(u64 a, u64 b) { return fq_sub(a, b); }
    static u64 mul(u64 a, u64 b) { return fq_mul(a, b); }
    static u64 inv(u64 a) { return fq_inv(a); }
    static u64 from_word(u64 x) { return x; }   // absorbed words enter the state as they are: every caller hands canonical words
};
class Transcript {
  public:
    Transcript();
    void absorb_fq(const u64 *x, size_t n);
    void absorb_ring(const u64 *elems, size_t count);     // Transcript::absorb / absorb_slice
    void absorb_label(const char *ascii);                 // absorb_field_element(from_be_bytes_mod_order(label))
    void absorb_fq3_as_ring(Fq3 c);                       // absorb(R::from(c))
    void absorb_u64_as_ring(u64 v);                       // absorb(R::from(v as u128))
    Fq3 get_challenge();                                  // squeeze tau words, absorb them back
    void get_short_challenge(u64 coeff_out[24]);          // TranscriptWithShortChallenges (Goldilocks set)
    static void permute(u64 st[24]);        // sparse-factorised partial rounds (same output); AVX-512 IFMA lanes when available
    static void permute_scalar(u64 st[24]); // the same factorisation, scalar (reference for the SIMD path)
    static void permute_plain(u64 st[24]);  // textbook definition, for the self-test
    static void params(const u64 **ark, const u64 **mds);
    // sponge state hand-over to / from the device sponge (lf_kernels.hip): 24 state words, rate index, mode (1 = squeezing)
    void get_state(u64 out[26]) const { sp_.get_state(out); }
    // External-basis hook (lf_set_ext_basis): while set, ring elements / challenges handed to absorb_ring / absorb_fq3_as_ring /
    // absorb_u64_as_ring are INTERNAL-basis words and are converted to the external basis before the sponge sees them, and get_challenge
    // returns the internal coordinates of the squeezed (external) challenge.  T, Ti: 3x3 row-major, ext = T int; nullptr = off.
    void set_basis(const u64 *T, const u64 *Ti) { bT_ = T; bTi_ = Ti; }
    void set_state(const u64 in[26]) { sp_.set_state(in); }

    void squeeze(u64 *out, size_t n);   // raw field elements of the sponge (lf_transcript_squeeze_bytes)

  private:
    poseidon::Sponge<FqField, &Transcript::permute> sp_;
    const u64 *bT_ = nullptr, *bTi_ = nullptr;
};

// ---- host policy of lf_step_host.h / lf_verify.h on this ring: small inline functions over a host ring it REFERS to (a context's, or the default one) ------
#pragma GCC visibility push(hidden)   // (not part of the ABI)
struct GoldV {
    static constexpr int RE = lf::RE, TAU = lf::TAU;
    static u64 modulus() { return LF_P; }
    typedef Fq3 Ext;
    typedef Transcript Tr;
    const HostRing &ring;
    void mul(const u64 *a, const u64 *b, u64 *o) const { ring.mul_ntt(a, b, o); }
    void mul_ext(const u64 *a, Ext s, u64 *o) const { ring.mul_fq3(a, s, o); }
    static void add(const u64 *a, const u64 *b, u64 *o) { HostRing::add(a, b, o); }
    static void sub(const u64 *a, const u64 *b, u64 *o) { HostRing::sub(a, b, o); }
    static void from_u64(u64 v, u64 *o) { HostRing::from_u64(v, o); }
    static void from_ext(Ext e, u64 *o) { HostRing::from_fq3(e, o); }
    static bool is_diag(const u64 *e, Ext *out) { return HostRing::is_diag(e, out); }
    static Ext ext_from_u64(u64 v) { return fq3_make(v % LF_P, 0, 0); }
    Ext ext_mul(Ext a, Ext b) const { return ring.mul3(a, b); }
    static Ext ext_add(Ext a, Ext b) { return fq3_add(a, b); }
    static Ext ext_sub(Ext a, Ext b) { return fq3_sub(a, b); }
    Ext ext_inv(Ext a) const { return ring.inv3(a); }
    static Ext ext_scale(Ext a, u64 k) { return fq3_make(fq_mul(a.c[0], k), fq_mul(a.c[1], k), fq_mul(a.c[2], k)); }   // times a base-field word
    static u64 finv(u64 a) { return fq_inv(a); }
    static void absorb_ext(Tr &tr, Ext e) { tr.absorb_fq3_as_ring(e); }
    void crt(const u64 *c, u64 *o) const { ring.crt(c, o); }
    void icrt(const u64 *x, u64 *o) const { ring.icrt(x, o); }
    static u64 fmul(u64 a, u64 b) { return fq_mul(a % LF_P, b % LF_P); }
    static u64 fadd(u64 a, u64 b) { return fq_add(a, b); }
    static u64 from_i64(int64_t v) { return fq_from_i64(v); }
    static void balanced_digits(u64 v, u64 base, unsigned digits, int64_t *out, int mode) { lf::balanced_digits(v, base, digits, out, mode); }
    // accumulation of the v_0 product (lfs::fold_v0): modular per term.  acc_mac takes any 64-bit words t (fq_mul reduces its operands and returns a canonical
    // word); the accumulators stay canonical
    typedef u64 Acc;
    static Acc acc_coef(u64 c) { return c % LF_P; }
    static void acc_mac(Acc *d, const u64 *t, int n, Acc r) { for (int x = 0; x < n; x++) d[x] = fq_add(d[x], fq_mul(t[x], r)); }
    static void acc_fold(Acc &mid, Acc &lo, Acc top) { mid = fq_add(mid, top); lo = fq_sub(lo, top); }   // X^d = X^(d - RE/2) - X^(d - RE)
    static u64 acc_word(Acc a) { return a; }
};
#pragma GCC visibility pop

}  // namespace lf
