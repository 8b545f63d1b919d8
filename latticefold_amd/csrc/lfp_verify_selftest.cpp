// lfp_verify_selftest.cpp -- lfplus_verify and lfplus_verify_ccs on malformed and on well-formed buffers, as a stand-alone host program for a sanitizer build (`make asan-verify`):
// lfp_prover.cpp and this file are compiled with -fsanitize=address,undefined and linked against the ordinary liblfhip.so for the three host verifiers and the
// transcript.  Every buffer is a heap allocation of exactly the length it claims, so a verifier that sized anything from the proof's header, or read past
// the end, stops the program.  No GPU is needed.  Prints one line per case and "selftest ok"; exit status 0 only when every case gave the expected code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/lfplus.h"

static int fails = 0;
static void expect(const char *name, int got, bool ok) {
    printf("%-28s rc = %d %s\n", name, got, ok ? "" : "UNEXPECTED");
    if (!ok) fails++;
}
static void refused(const char *name, int got) { expect(name, got, got == LFPLUS_E_ARG); }
// the call on a buffer of exactly `words` words (copied from src, zero-filled beyond it)
static int run(const lfplus_params &p, uint64_t n, uint32_t nM, uint32_t L, uint32_t nfresh, const std::vector<uint64_t> &src, size_t words, bool null_proof = false) {
    uint64_t *buf = (uint64_t *)calloc(words ? words : 1, 8);
    memcpy(buf, src.data(), (words < src.size() ? words : src.size()) * 8);
    lfplus_transcript *t = lfplus_transcript_new();
    int which = 0, stage = 0;
    const int rc = lfplus_verify(&p, n, nM, L, nfresh, t, null_proof ? nullptr : buf, words, &which, &stage);
    lfplus_transcript_free(t);
    free(buf);
    return rc;
}
// lfplus_verify_ccs the same way: a gate over four matrices (t 4, q 3, d 3, seven indices), L = 2, one fresh instance
static int run_ccs(const lfplus_params &p, uint64_t n, const lfplus_ccs *s, uint32_t L, uint32_t nfresh, const std::vector<uint64_t> &src, size_t words, bool null_proof = false) {
    uint64_t *buf = (uint64_t *)calloc(words ? words : 1, 8);
    memcpy(buf, src.data(), (words < src.size() ? words : src.size()) * 8);
    lfplus_transcript *t = lfplus_transcript_new();
    int which = 0, stage = 0;
    const int rc = lfplus_verify_ccs(&p, n, s, L, nfresh, t, null_proof ? nullptr : buf, words, &which, &stage);
    lfplus_transcript_free(t);
    free(buf);
    return rc;
}
static void ccs_cases(const lfplus_params &p, uint64_t n) {
    const uint32_t S_off[4] = {0, 3, 5, 7}, S_idx[7] = {0, 1, 2, 3, 0, 3, 3}, L = 2, nfresh = 1;
    uint64_t c[3 * 16] = {0};
    c[0] = 1; c[16] = LFPLUS_P - 1; c[32 + 5] = 12345;      // 1, -1, a general coefficient
    const lfplus_ccs s = {4, 3, S_off, S_idx, c};
    const uint64_t len = lfplus_proof_len_ccs(&p, n, &s, L, nfresh);
    if (!len) { printf("lfplus_proof_len_ccs refused the shape\n"); fails++; return; }
    std::vector<uint64_t> good(len, 0);
    const uint64_t hdr[LFPLUS_PROOF_HEADER_CCS] = {LFPLUS_PROOF_MAGIC_CCS, L, nfresh, 6, p.k, p.l, p.kappa, 4, 3, 3, 7, 0};
    memcpy(good.data(), hdr, sizeof hdr);
    int rc = run_ccs(p, n, &s, L, nfresh, good, len);
    expect("ccs: well-formed zeros", rc, rc == LFPLUS_OK || rc == LFPLUS_E_REJECT);
    for (uint64_t i = LFPLUS_PROOF_HEADER_CCS; i < len; i++) good[i] = (i * 0x9E3779B97F4A7C15ull) % LFPLUS_P;
    rc = run_ccs(p, n, &s, L, nfresh, good, len);
    expect("ccs: well-formed words", rc, rc == LFPLUS_E_REJECT);
    refused("ccs: one word short", run_ccs(p, n, &s, L, nfresh, good, len - 1));
    refused("ccs: one word long", run_ccs(p, n, &s, L, nfresh, good, len + 1));
    refused("ccs: header only", run_ccs(p, n, &s, L, nfresh, good, LFPLUS_PROOF_HEADER_CCS));
    refused("ccs: NULL proof", run_ccs(p, n, &s, L, nfresh, good, len, true));
    for (int w = 0; w < LFPLUS_PROOF_HEADER_CCS; w++) {
        std::vector<uint64_t> bad(good);
        bad[w] += 1;
        refused("ccs: a header word + 1", run_ccs(p, n, &s, L, nfresh, bad, len));
    }
    {   // the R1CS buffer of the same statement (shorter, other magic), and this buffer under a statement with a longer one
        const uint64_t len3 = lfplus_proof_len(&p, n, 4, L, nfresh);
        std::vector<uint64_t> r(len3, 0);
        const uint64_t h3[LFPLUS_PROOF_HEADER] = {LFPLUS_PROOF_MAGIC, L, nfresh, 6, p.k, p.l, p.kappa, 4};
        memcpy(r.data(), h3, sizeof h3);
        refused("ccs: an R1CS-layout buffer", run_ccs(p, n, &s, L, nfresh, r, len3));
        refused("ccs: statement larger than buffer", run_ccs(p, n, &s, L + 1, nfresh, good, len));
    }
    const uint32_t bad_idx[7] = {0, 1, 2, 3, 0, 3, 4};      // an index >= t: refused as a shape, the (well-formed) buffer is not read
    const lfplus_ccs s2 = {4, 3, S_off, bad_idx, c};
    refused("ccs: index >= t", run_ccs(p, n, &s2, L, nfresh, good, len));
    refused("ccs: NULL shape", run_ccs(p, n, nullptr, L, nfresh, good, len));
    expect("ccs: len of a bad shape", (int)lfplus_proof_len_ccs(&p, n, &s2, L, nfresh), lfplus_proof_len_ccs(&p, n, &s2, L, nfresh) == 0);
}
int main() {
    const lfplus_params p = {1, 2, 2, 8, 7};      // kappa, k, l, b, B
    const uint64_t n = 64;
    const uint32_t nM = 1, L = 2, nfresh = 1;
    const uint64_t len = lfplus_proof_len(&p, n, nM, L, nfresh);
    if (!len) { printf("lfplus_proof_len refused the shape\n"); return 2; }
    std::vector<uint64_t> good(len, 0);
    const uint64_t hdr[LFPLUS_PROOF_HEADER] = {LFPLUS_PROOF_MAGIC, L, nfresh, 6, p.k, p.l, p.kappa, nM};
    memcpy(good.data(), hdr, sizeof hdr);
    // a well-formed buffer (all-zero fields): the three sub-verifiers run over every field they read; it is a verdict, not a refusal
    int rc = run(p, n, nM, L, nfresh, good, len);
    expect("well-formed zeros", rc, rc == LFPLUS_OK || rc == LFPLUS_E_REJECT);
    for (uint64_t i = LFPLUS_PROOF_HEADER; i < len; i++) good[i] = (i * 0x9E3779B97F4A7C15ull) % LFPLUS_P;
    rc = run(p, n, nM, L, nfresh, good, len);
    expect("well-formed words", rc, rc == LFPLUS_E_REJECT);
    refused("one word short", run(p, n, nM, L, nfresh, good, len - 1));
    refused("one word long", run(p, n, nM, L, nfresh, good, len + 1));
    refused("header only", run(p, n, nM, L, nfresh, good, LFPLUS_PROOF_HEADER));
    refused("empty", run(p, n, nM, L, nfresh, good, 0));
    refused("NULL proof", run(p, n, nM, L, nfresh, good, len, true));
    for (int w : {1, 6}) {      // header words L and kappa disagree with the arguments
        std::vector<uint64_t> bad(good);
        bad[w] += 1;
        refused(w == 1 ? "header L + 1" : "header kappa + 1", run(p, n, nM, L, nfresh, bad, len));
    }
    {   // a buffer as long as its LYING header implies (kappa 2, L 3) under the verifier's own statement
        lfplus_params q = p;
        q.kappa = 2;
        const uint64_t len2 = lfplus_proof_len(&q, n, nM, 3, nfresh);
        std::vector<uint64_t> lie(len2, 0);
        const uint64_t h2[LFPLUS_PROOF_HEADER] = {LFPLUS_PROOF_MAGIC, 3, nfresh, 6, q.k, q.l, q.kappa, nM};
        memcpy(lie.data(), h2, sizeof h2);
        refused("longer, lying header", run(p, n, nM, L, nfresh, lie, len2));
        // the SHORT buffer under a statement that implies a longer one: nothing beyond its end may be read
        refused("statement larger than buffer", run(q, n, nM, 3, nfresh, good, len));
    }
    refused("outside the envelope", run(p, n + 1, nM, L, nfresh, good, len));
    ccs_cases(p, n);
    if (fails) { printf("%d case(s) failed\n", fails); return 1; }
    printf("selftest ok\n");
    return 0;
}
