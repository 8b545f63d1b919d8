// lfp_poseidon_simd.h -- AVX-512 IFMA lanes for the host side of the LatticeFold+ Fiat-Shamir transcript (PoseidonTranscript<RqPoly> on the Frog ring,
// crates/latticefold-plus/src/transcript.rs:20-78; width 24, 8 full + 22 partial rounds, x^7) over a GENERIC 64-bit prime: Montgomery words with
// R = 2^104, 64x64-bit products as 52-bit limb products (vpmadd52luq / vpmadd52huq) accumulated without carries, one two-step radix-2^52 Montgomery
// reduction per output word; the partial rounds collapsed into two mat-vecs and a scalar chain (poseidon::collapse_partial).  A prove at 2^20 rows makes
// ~2 000 permutations on the critical path of the host (set-check challenges, 120 sumcheck rounds, the evaluations' absorb): the scalar form
// (FastPerm, lfp_protocol.cpp) costs 7-12 us each.  Same output as FastPerm::run / permute_plain (tests/test_oracle_lfp_protocol.py, test_abi_cpu.py).
// Selected at run time (cpuid); LFPLUS_POSEIDON_SCALAR=1 forces the scalar path.
#pragma once
#include "poseidon_host.h"

namespace lfp_psimd {

// both only where poseidon::avx512_ifma_supported()
void build(uint64_t p, const poseidon::Table &t, const poseidon::Collapsed &c);   // the prime, its table and collapsed partial rounds (canonical words)
void permute(uint64_t st[24]);   // canonical words in and out

}  // namespace lfp_psimd
