// lf_witness_parts.h -- the K decomposed witnesses of a witness handle as handles of their own (decompose_witness, nifs/decomposition.rs:162-167) and the way
// back: launchers of lf_witness_parts.hip.  A witness is int32 planes [RE][N] on both rings and the digit rule acts on one coefficient at a time, so the kernels
// see a flat array of `total` = RE * N centred coefficients: one body, the ring is data.
// Every launcher returns 0, or -1 when the arguments are outside what the kernels take or the launch failed.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lfparts {

constexpr uint32_t MAX_PARTS = 32;   // part pointers travel by value in the kernel arguments

// bits of the flag word of launch_witness_join; FLAG_NORM / FLAG_NO_I32 are the bits k_coef_to_i32 raises (lf_ring_kernels.cuh)
enum : uint32_t {
    FLAG_NORM = 1,            // the sum exceeds the ingest bound
    FLAG_NO_I32 = 2,          // the sum is +2^31 (within the bound at B = 2^32 only): an int32 plane cannot hold it
    FLAG_DIGIT = 4,           // a digit outside the rule's range
    FLAG_NOT_CANONICAL = 8,   // legal digits that are not the decomposition of their own sum (a tie on the wrong side, a non-zero last carry)
};

// parts[k][i] = digit k of planes[i] under the digit rule `mode` (lfdec::DigitChain), base 2^lb, k < K <= MAX_PARTS.  Every pointer 16-byte aligned.
int launch_witness_cut(const int32_t *planes, size_t total, uint32_t K, uint32_t lb, int mode, int32_t *const *parts, hipStream_t s);
// planes[i] = sum_k 2^(lb k) parts[k][i] where the K digits are legal and are the decomposition of that sum and |sum| <= bound fits an int32; 0 and a bit of
// *flag (lowered by the caller, in stream) otherwise.  K * lb <= 60.
int launch_witness_join(const int32_t *const *parts, size_t total, uint32_t K, uint32_t lb, int mode, uint64_t bound, int32_t *planes, uint32_t *flag,
                        hipStream_t s);

}  // namespace lfparts
