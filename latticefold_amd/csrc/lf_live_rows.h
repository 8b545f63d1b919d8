// lf_live_rows.h -- host only: the trailing run of empty rows of the constraint matrices and the schedule by which the linearization skips it.
//
// lf_ccs_load wants N = wit_len * L <= m = 2^s (sanity_check, nifs.rs:165-173) and the matrices are padded with empty rows up to m: a system has about as many
// constraints as variables, so with L > 1 only the first ~ n = l + 1 + wit_len rows of every M_j have entries.  An empty row is a zero of every M_j z table, and
// a zero entry contributes exactly 0 to every point of every round message of the linearization sumcheck (each multiset product has a zero factor) and fixes to 0.
// Field sums are exact, so leaving those terms out gives the same words.
//
// live_rows = 1 + the last row with an entry in any M_j (0: all matrices empty).  Only the TRAILING run is cut: empty rows in between are ordinary rows.
// The linearization works on a padded prefix:  pad = live_rows rounded up to the granule g = 2^k (at least g), so that the live counts halve exactly
// through k rounds -- round i (1-based) has n_i = m >> (i-1) entries per table, of which the first pad >> (i-1) are live while 2^i divides pad (whole pairs in
// round i and an exact half for round i + 1: ceilings would accumulate otherwise).  From the first round where that fails the tables are whole again (the driver
// zero-fills the rest of the M z tables once: run_lin_sumcheck).  Only the M z tables are cut: the eq factor is dense and stays whole.
// Threshold: the prefix is used when pad <= m / 2 (at least half of every pass over the M z tables is saved; what it adds is one small pass over the rest of
// the eq table per round and one memset at the hand-over) and m >= min_m; otherwise pad == m and every launch is the whole-table one.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lflive {

static constexpr size_t GRANULE = 4096;        // default granule: 2048 pairs = 8 blocks of a round kernel; twelve exact halvings, beyond the persistent tail's size
static constexpr size_t MIN_M = (size_t)1 << 14;   // below, a round is a ~30 us launch whatever its length
static constexpr size_t GRANULE_LOW = 8, MIN_M_LOW = 16;   // LF_LIVE_ROWS_LOW: tiny shapes exercise the truncated rounds (tests)

// 1 + the last row r with rowptr[j][r + 1] > rowptr[j][r] for any j < t; 0 if every row of every matrix is empty
static inline size_t live_rows(unsigned t, size_t m, const uint32_t *const *rowptr) {
    size_t live = 0;
    for (unsigned j = 0; j < t; j++) {
        size_t r = m;
        while (r > live && rowptr[j][r] == rowptr[j][r - 1]) r--;   // (monotone row pointers: the first difference from the end is the last non-empty row)
        if (r > live) live = r;
    }
    return live;
}

struct Plan {
    size_t m = 0;
    size_t pad = 0;   // live entries of the round-1 tables (== m: no truncation)
    bool on() const { return pad < m; }
};
// m, granule: powers of two
static inline Plan plan(size_t m, size_t live, size_t granule, size_t min_m) {
    Plan p;
    p.m = m; p.pad = m;
    if (granule < 4 || (granule & (granule - 1)) || m < min_m || live > m) return p;
    size_t pad = (live + granule - 1) / granule * granule;
    if (pad < granule) pad = granule;
    if (pad <= m / 2) p.pad = pad;
    return p;
}
// may tables of `n` entries of which the first `nl` are live be halved into truncated ones?  (the fused round reads entries 4p .. 4p+3, p < nl / 4)
static inline bool halves(size_t n, size_t nl) { return nl < n && nl % 4 == 0 && nl >= 4; }
// live entries of the tables of round i (1-based) under the plan alone (the driver may stop earlier: persistent tail, small non-fused rounds)
static inline size_t entries(const Plan &p, unsigned round) {
    size_t n = p.m, nl = p.pad;
    for (unsigned i = 1; i < round; i++) {
        nl = halves(n, nl) ? nl / 2 : n / 2;
        n /= 2;
    }
    return nl;
}

}   // namespace lflive
