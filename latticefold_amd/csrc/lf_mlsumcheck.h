// lf_mlsumcheck.h -- the generic sumcheck over a sum of products of MLE tables (lf_mlsumcheck_*, include/lfhip_sumcheck.h): the descriptor as the round kernel
// takes it and the launchers of lf_mlsumcheck.hip, one overload per ring (resolved by the table struct, as every other launcher of lf_ring_host.h).
//   g(x) = sum_{i < q} coef_i * prod_{k in [off[i], off[i+1])} T_{idx[k]}(x)      (VirtualPolynomial, utils/sumcheck/utils.rs:24-75)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lf { struct DevCrt; }
namespace lfbb { struct DevBb; }   // (the table structs of the two rings, lf_kernels.h / bb_kernels.h: the launchers below resolve by them)

namespace lfml {

constexpr uint32_t MAX_NVARS = 30;     // LF_S_MAX: the longest table any entry point takes
constexpr uint32_t MAX_TABLES = 16, MAX_TERMS = 16, MAX_FACTORS = 8, MAX_IDX = 64, MAX_DEGREE = 8;
constexpr uint32_t MAX_BLOCKS = 256;   // blocks of 256 pairs a round strides over the pairs with (per slot and point group): rows of the partial buffer
// points a block evaluates (the degree + 1 points of a round are split over blockIdx.z in groups of this size): the running products and the sums of a
// group live in named registers, so the size is a compile-time constant per ring -- 4 words of F_{p^3} (degree 3, the linearization shape, is one group), 3 of
// F_{p^9} (nine words each)
constexpr uint32_t PTS_GOLD = 4, PTS_BB = 3;

// class of a coefficient in one CRT slot: what the kernel does with a term's product there
enum : uint32_t { COEF_ZERO = 0, COEF_ONE = 1, COEF_MINUS_ONE = 2, COEF_GENERAL = 3 };

// The FIRST kernel argument of k_mls_round: the kernel reads it through the kernel-argument segment (scalar loads), never as an indexed by-value struct.
// The coefficients' slot words do not fit beside it (16 x 72 words on BabyBear against a 4 KB segment): they stay in a buffer of the context and are read with
// wave-uniform addresses, once per term and only where the class says COEF_GENERAL.
struct Desc {
    uint32_t q, npts;               // terms; degree + 1
    uint32_t cls[MAX_TERMS];        // 2 bits per slot: COEF_* of term i in slot s at bits [2s, 2s + 2)
    uint32_t off[MAX_TERMS + 1];    // term i = factors off[i] .. off[i + 1]
    uint32_t idx4[MAX_IDX / 4];     // table of factor k: byte k % 4 of word k / 4 (whole words: the scalar unit loads nothing narrower)
    void set_idx(uint32_t k, uint32_t table) { idx4[k / 4] |= table << (8 * (k % 4)); }
};

inline uint32_t round_blocks(size_t npairs) {
    const size_t b = (npairs + 255) / 256;
    return (uint32_t)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}
inline uint32_t point_groups(uint32_t npts, uint32_t pts) { return (npts + pts - 1) / pts; }
// words of the partial buffer of a round (Part words: u64 on Goldilocks, i64 on BabyBear): one row of (groups * pts) evaluations per block
inline size_t partial_words(uint32_t pts, uint32_t re) { return (size_t)MAX_BLOCKS * point_groups(MAX_DEGREE + 1, pts) * pts * re; }

// One round message: tab = T tables [RE][ld] of n = 2 npairs entries, coef = q x RE device words (the ring's device form), out = npts x RE canonical words
// (AoS ring elements).  0, or -1 when the launch failed.
int launch_mls_round(const lf::DevCrt &t, const Desc &d, const uint64_t *tab, size_t ld, size_t npairs, const uint64_t *coef, uint64_t *partial, uint64_t *out,
                     hipStream_t s);
int launch_mls_round(const lfbb::DevBb &t, const Desc &d, const int32_t *tab, size_t ld, size_t npairs, const int32_t *coef, int64_t *partial, uint64_t *out,
                     hipStream_t s);

}  // namespace lfml
