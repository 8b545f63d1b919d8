// poseidon_host.h -- the host Poseidon of the three Fiat-Shamir transcripts (Goldilocks lf::Transcript, BabyBear lfbb::BbTranscript, Frog
// lfplus_transcript), once: shape, parameter table, the textbook permutation, the table builders of the fast permutations and the duplex sponge.
// All three rings use the same construction -- width 24 = rate 20 + capacity 4, 8 full + 22 partial rounds, alpha = 7, the arkworks-0.4
// PoseidonSponge (duplex) -- and the same parameters: the Grain-LFSR table generated for the 64-bit Goldilocks prime (lf_host.cpp), embedded
// into each field with Fq::from(i128), i.e. reduced mod p (rings/poseidon/{goldilocks,babybear,frog}.rs:7-1425).
//
// Everything here works on CANONICAL u64 words and is parameterised by a field policy F:
//     static constexpr u64 P;                         the prime
//     static u64 add(a, b), sub(a, b), mul(a, b), inv(a);   canonical in, canonical out
//     static u64 from_word(x);                        an input word of absorb() as it enters the state
// (lf::FqField in lf_host.h, lfbb::BbField in bb_host.h, the Frog policy in lfp_protocol.cpp).  What is NOT here is the tuned arithmetic of the
// permutations that actually run: the scalar sparse forms (Transcript::permute_scalar, BbTranscript::permute_scalar, FastPerm::run) and the
// SIMD lanes (lf_poseidon_simd.cc, bb_poseidon_avx512.cc, bb_poseidon_simd.h, lfp_poseidon_simd.cc) differ per prime for measured reasons;
// they take the canonical tables built here and convert them into their own word forms.
// Plain host C++ (no HIP, no intrinsics): the plain-data part is also included by the AVX-512 translation units.  The templates are to be
// instantiated from the ordinary host translation units only (the AVX-512 units are built with other target flags).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

namespace poseidon {
typedef uint64_t u64;
constexpr int W = 24, RATE = 20, CAP = 4, RF = 8, RP = 22;

inline bool avx512_ifma_supported() {   // what the three AVX-512 IFMA translation units need of this CPU
    static const bool ok = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512ifma") && __builtin_cpu_supports("avx512dq");
    return ok;
}

// ---- parameters ----------------------------------------------------------------------------------------------------------------------------
struct Table {
    u64 ark[(RF + RP) * W];   // round constants, round-major
    u64 mds[W * W];           // row-major
};
const Table &grain_table();   // the Grain-LFSR output (n = 64, t = 24, R_F = 8, R_P = 22) over the Goldilocks prime: lf_host.cpp
template <class F>
void reduced_table(Table &t) {   // the table of the field F
    const Table &g = grain_table();
    for (int i = 0; i < (RF + RP) * W; i++) t.ark[i] = g.ark[i] % F::P;
    for (int i = 0; i < W * W; i++) t.mds[i] = g.mds[i] % F::P;
}

template <class F>
inline u64 sbox(u64 x) {
    const u64 x2 = F::mul(x, x), x3 = F::mul(x2, x), x4 = F::mul(x2, x2);
    return F::mul(x4, x3);
}
template <class F>
inline u64 dot(const u64 *a, const u64 *b, int n, int stride_b = 1) {
    u64 acc = 0;
    for (int k = 0; k < n; k++) acc = F::add(acc, F::mul(a[k], b[(size_t)k * stride_b]));
    return acc;
}

// the definition (ark-crypto-primitives PoseidonSponge::permute): the reference every fast form is tested against
template <class F>
void permute_plain(const Table &t, u64 st[W]) {
    u64 nw[W];
    for (int r = 0; r < RF + RP; r++) {
        const u64 *ark = t.ark + r * W;
        const bool full = r < RF / 2 || r >= RF / 2 + RP;
        for (int i = 0; i < W; i++) st[i] = F::add(st[i], ark[i]);
        if (full) for (int i = 0; i < W; i++) st[i] = sbox<F>(st[i]);
        else st[0] = sbox<F>(st[0]);
        for (int i = 0; i < W; i++) nw[i] = dot<F>(st, t.mds + i * W, W);
        memcpy(st, nw, sizeof(nw));
    }
}

// ---- sparse partial rounds -----------------------------------------------------------------------------------------------------------------
template <class F>
bool mat_inv(const u64 *in, u64 *out, int n) {   // Gauss-Jordan over F_p; false: singular
    std::vector<u64> M((size_t)n * 2 * n, 0);
    for (int r = 0; r < n; r++) {
        for (int c = 0; c < n; c++) M[(size_t)r * 2 * n + c] = in[r * n + c];
        M[(size_t)r * 2 * n + n + r] = 1;
    }
    for (int col = 0; col < n; col++) {
        int piv = -1;
        for (int r = col; r < n; r++)
            if (M[(size_t)r * 2 * n + col]) { piv = r; break; }
        if (piv < 0) return false;
        if (piv != col)
            for (int c = 0; c < 2 * n; c++) std::swap(M[(size_t)piv * 2 * n + c], M[(size_t)col * 2 * n + c]);
        const u64 inv = F::inv(M[(size_t)col * 2 * n + col]);
        for (int c = 0; c < 2 * n; c++) M[(size_t)col * 2 * n + c] = F::mul(M[(size_t)col * 2 * n + c], inv);
        for (int r = 0; r < n; r++) {
            const u64 f = M[(size_t)r * 2 * n + col];
            if (r == col || !f) continue;
            for (int c = 0; c < 2 * n; c++) M[(size_t)r * 2 * n + c] = F::sub(M[(size_t)r * 2 * n + c], F::mul(f, M[(size_t)col * 2 * n + c]));
        }
    }
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) out[r * n + c] = M[(size_t)r * 2 * n + n + c];
    return true;
}

// Partial rounds through the sparse factorisation M*diag(1,E) = diag(1,E') * [[e00, row],[col, I]] (Poseidon paper, appendix on optimised
// partial rounds): identical output, 47 instead of 576 multiplications per partial round.  Round r is
//     state += cst[r];  x0 = sbox(state[0]);  state[0] = e00[r] x0 + row[r] . state[1..];  state[1..] += col[r] x0
// and state[1..] = post state[1..] once after the last one.
struct Sparse {
    u64 cst[RP][W];       // round constants pulled through the deferred block-diagonal factor
    u64 e00[RP];
    u64 row[RP][W - 1];
    u64 col[RP][W - 1];
    u64 post[W - 1][W - 1];  // deferred factor applied once after the last partial round
};
template <class F>
bool sparse_partial(const Table &t, Sparse &s) {   // false: a block is singular and the factorisation does not exist (s is then unusable)
    const int n = W - 1;
    std::vector<u64> Eprev((size_t)n * n, 0), EprevInv((size_t)n * n, 0), eff((size_t)W * W), Eh((size_t)n * n), Ei((size_t)n * n);
    for (int i = 0; i < n; i++) Eprev[(size_t)i * n + i] = EprevInv[(size_t)i * n + i] = 1;
    for (int r = 0; r < RP; r++) {
        const u64 *c = t.ark + (size_t)(RF / 2 + r) * W;
        // constants: c' = diag(1, Eprev^-1) c
        s.cst[r][0] = c[0];
        for (int i = 0; i < n; i++) s.cst[r][1 + i] = dot<F>(&EprevInv[(size_t)i * n], c + 1, n);
        // eff = M * diag(1, Eprev)
        for (int i = 0; i < W; i++) {
            eff[(size_t)i * W] = t.mds[i * W];
            for (int j = 0; j < n; j++) eff[(size_t)i * W + 1 + j] = dot<F>(t.mds + i * W + 1, &Eprev[j], n, n);
        }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) Eh[(size_t)i * n + j] = eff[(size_t)(1 + i) * W + 1 + j];
        if (!mat_inv<F>(Eh.data(), Ei.data(), n)) return false;
        s.e00[r] = eff[0];
        for (int j = 0; j < n; j++) s.row[r][j] = eff[1 + j];
        for (int i = 0; i < n; i++) s.col[r][i] = dot<F>(&Ei[(size_t)i * n], &eff[W], n, W);
        Eprev = Eh;
        EprevInv = Ei;
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) s.post[i][j] = Eprev[(size_t)i * n + j];
    return true;
}

// ---- the sparse rounds collapsed by linearity (the form of the AVX-512 IFMA lanes) -----------------------------------------------------------
//   D = SX x (one mat-vec up front),  X_r = sbox(s0_r + cst0[r]),  s0_{r+1} = D_r + K_r + sum_{i<=r} G[r][i] X_i (scalar chain over word 0),
//   state' = FIN [x ; X] + fk (one closing mat-vec; word 0 of state' is the chain's last value s0_22).
// The mat-vec of the full round in front of the partial rounds (x = M s) is folded into what consumes its output: D = (SX M) s, the closing
// map's state part (FIN_x M) s, word 0 = (row 0 of M) s -- two mat-vecs over s instead of three.
constexpr int NX = W + RP;   // columns of the closing map: 24 state words + 22 S-box outputs
struct Collapsed {
    u64 sx[W][W];      // [j][r] = coefficient of state word j in D_r (row 0 and columns >= 22 zero)
    u64 cst0[RP];      // constant of word 0
    u64 G[RP][RP];     // lower triangle
    u64 K[RP];
    u64 Kc[RP];        // K_r + cst0[r + 1]: the next round's constant of word 0 rides along
    u64 fin[NX][W];    // [j][i]: closing map, columns 0..23 the state words, 24..45 the S-box outputs X_r; row 0 and lane 0 zero
    u64 fk[W];         // its constant; lane 0 zero
    u64 sxm[W][W];     // [j][r] = (SX M)[r][j] for r < 22, and row 0 of M in lane 22
    u64 finm[W][W];    // [j][i] = (FIN_x M)[i][j]
};
template <class F>
void collapse_partial(const Table &t, const Sparse &s, Collapsed &c) {
    memset(&c, 0, sizeof(c));
    // Symbolic run of the 22 sparse partial rounds.  Every state word 1..23 is an affine form over
    //   [ x_1..x_23 (words on entry) | X_0..X_21 (S-box outputs of word 0) | 1 ]
    // because a partial round is  xs = state[1..] + cst_r,  X_r = sbox(s0 + c0_r),  s0' = e00_r X_r + row_r . xs,
    // state'[1..] = xs + col_r X_r -- linear except for the S-box.  Collecting coefficients gives SX, G, K and
    //   state' = diag(1, post) [s0_22 ; x + CX X + ck].
    const int n = W - 1, NB = n + RP + 1;   // basis size
    std::vector<u64> formv((size_t)n * NB, 0);
    u64(*form)[W - 1 + RP + 1] = (u64(*)[W - 1 + RP + 1]) formv.data();
    for (int i = 0; i < n; i++) { form[i][i] = 1; form[i][NB - 1] = s.cst[0][1 + i]; }
    for (int r = 0; r < RP; r++) {
        c.cst0[r] = s.cst[r][0];
        u64 dotf[W - 1 + RP + 1];
        for (int b = 0; b < NB; b++) dotf[b] = dot<F>(s.row[r], &form[0][b], n, NB);
        for (int j = 0; j < n; j++) c.sx[1 + j][r] = dotf[j];
        for (int i = 0; i < r; i++) c.G[r][i] = dotf[n + i];
        c.G[r][r] = s.e00[r];
        c.K[r] = dotf[NB - 1];
        for (int i = 0; i < n; i++) {
            form[i][n + r] = F::add(form[i][n + r], s.col[r][i]);
            if (r + 1 < RP) form[i][NB - 1] = F::add(form[i][NB - 1], s.cst[r + 1][1 + i]);
        }
    }
    for (int r = 0; r < RP; r++) c.Kc[r] = r + 1 < RP ? F::add(c.K[r], c.cst0[r + 1]) : c.K[r];
    // closing map: words 1..23 = post * form
    for (int i = 0; i < n; i++)
        for (int b = 0; b < NB; b++) {
            const u64 a = dot<F>(s.post[i], &form[0][b], n, NB);
            if (b < n) c.fin[1 + b][1 + i] = a;
            else if (b < n + RP) c.fin[W + (b - n)][1 + i] = a;
            else c.fk[1 + i] = a;
        }
    for (int j = 0; j < W; j++)
        for (int r = 0; r < W; r++) {
            u64 a = 0, b = 0;
            for (int i = 0; i < W; i++) {
                a = F::add(a, F::mul(c.sx[i][r], t.mds[i * W + j]));
                b = F::add(b, F::mul(c.fin[i][r], t.mds[i * W + j]));
            }
            c.sxm[j][r] = r == RP ? t.mds[0 * W + j] : a;
            c.finm[j][r] = b;
        }
}

// ---- duplex sponge (ark-crypto-primitives 0.4.0 PoseidonSponge): state[0..4) capacity, [4..24) rate ---------------------------------------------
template <class F, void (*Permute)(u64 *)>
struct Sponge {
    u64 st[W] = {0};
    bool squeezing = false;
    int idx = 0;          // next rate word of the current mode
    void absorb(const u64 *x, size_t n) {
        if (!n) return;
        int i0;
        if (!squeezing) {
            i0 = idx;
            if (i0 == RATE) { Permute(st); i0 = 0; }
        } else {
            Permute(st);
            i0 = 0;
        }
        for (;;) {
            if ((size_t)i0 + n <= (size_t)RATE) {
                for (size_t i = 0; i < n; i++) st[CAP + i0 + i] = F::add(st[CAP + i0 + i], F::from_word(x[i]));
                squeezing = false;
                idx = i0 + (int)n;
                return;
            }
            const size_t take = RATE - i0;
            for (size_t i = 0; i < take; i++) st[CAP + i0 + i] = F::add(st[CAP + i0 + i], F::from_word(x[i]));
            Permute(st);
            x += take; n -= take; i0 = 0;
        }
    }
    void squeeze(u64 *out, size_t n) {
        int i0;
        if (!squeezing) { Permute(st); i0 = 0; }
        else {
            i0 = idx;
            if (i0 == RATE) { Permute(st); i0 = 0; }
        }
        for (;;) {
            if ((size_t)i0 + n <= (size_t)RATE) {
                memcpy(out, st + CAP + i0, n * sizeof(u64));
                squeezing = true;
                idx = i0 + (int)n;
                return;
            }
            const size_t take = RATE - i0;
            memcpy(out, st + CAP + i0, take * sizeof(u64));
            if (n != (size_t)RATE) Permute(st);   // arkworks: no permutation when exactly one block remains (the next call starts with a full index)
            out += take; n -= take; i0 = 0;
        }
    }
    // hand-over to / from a sponge that runs elsewhere (the device sponge): 24 state words, rate index, mode (1 = squeezing)
    void get_state(u64 out[W + 2]) const { for (int i = 0; i < W; i++) out[i] = st[i]; out[W] = (u64)idx; out[W + 1] = squeezing ? 1 : 0; }
    void set_state(const u64 in[W + 2]) { for (int i = 0; i < W; i++) st[i] = in[i]; idx = (int)in[W]; squeezing = in[W + 1] != 0; }
};

}  // namespace poseidon
