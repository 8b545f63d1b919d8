// lf_capi.cpp -- the C ABI (include/lfhip.h) of the Goldilocks backend, part 1: context, ring tables, sharding / RCCL set-up, staging, the component entry
// points (CRT, decomposition, Ajtai commitments, eq tables, MLE evaluations, SpMV), constraint-system load, device-resident witnesses, transcripts, timing
// read-outs and the host verifier.  The provers are in lf_prove.cpp (linearization, decomposition, entry points) and lf_fold.cpp (the folding prover).
#include "lf_ring_host.h"
#include <thread>
#include <vector>

const char *lf_strerror(int code) {
    switch (code) {
        case LF_OK: return "ok";
        case LF_ERR_INVALID: return "invalid argument / wrong length";
        case LF_ERR_HIP: return "HIP runtime error (no GPU or out of device memory)";
        case LF_ERR_UNSUPPORTED: return "unsupported parameter";
        case LF_ERR_BAD_TABLES: return "ring tables are not a ring isomorphism";
        case LF_ERR_NORM: return "witness coefficient exceeds the decomposition bound";
        case LF_ERR_SIZE_BOUNDS: return "invalid size bounds (m must be >= wit_len*L, power of two)";
        case LF_ERR_STATE: return "call sequence misuse";
        case LF_ERR_REJECT: return "verifier rejected the proof";
    }
    return "unknown error";
}
const char *lf_phase_name(int i) { return (i >= 0 && i < LF_N_PHASES) ? PHASE_NAMES[i] : ""; }

// ---------------------------------------------------------------------------------------------------------------
static int install_tables(lf_ctx *c, u64 nonres, const u64 *y) {
    CrtTables T;
    if (build_crt_tables(nonres, y, T) != 0) return LF_ERR_BAD_TABLES;
    c->ring.T = T;
    c->dcrt = make_dev_crt(T);
    c->zk_i8.state = 0;   // (the int8 matrix of the z_k build belongs to the tables: built again at its next use)
    return ring_ops<GoldRing>::install_icrt(c, &T.icrt[0][0]);
}

int lf_ctx_create_ring(lf_ctx **out, int device, int ring) {
    if (ring == LF_RING_GOLDILOCKS) return lf_ctx_create(out, device);
    if (!out || ring != LF_RING_BABYBEAR) return LF_ERR_INVALID;
    lf_ctx *c = new lf_ctx();
    c->device = device;
    int rc = lfbb::BbCtx::create(&c->bb, c, device);
    if (rc != LF_OK) { delete c; return rc; }
    *out = c;
    return LF_OK;
}
int lf_ctx_device(const lf_ctx *c) { return c->device; }
int lf_ctx_ring(const lf_ctx *c) { return c && c->bb ? LF_RING_BABYBEAR : LF_RING_GOLDILOCKS; }
int lf_ring_words(int ring) { return ring == LF_RING_BABYBEAR ? 72 : (ring == LF_RING_GOLDILOCKS ? 24 : 0); }
int lf_ring_tau(int ring) { return ring == LF_RING_BABYBEAR ? 9 : (ring == LF_RING_GOLDILOCKS ? 3 : 0); }
uint64_t lf_ring_modulus(int ring) { return ring == LF_RING_BABYBEAR ? (uint64_t)lfbb::BB_P : (ring == LF_RING_GOLDILOCKS ? LF_P : 0); }

int lf_ctx_create(lf_ctx **out, int device) {
    if (!out) return LF_ERR_INVALID;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0 || device < 0 || device >= cnt) return LF_ERR_HIP;
    HIPCHK(hipSetDevice(device));
    lf_ctx *c = new lf_ctx();
    c->device = device;
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (c->create_lane_streams() != LF_OK || hipStreamCreateWithPriority(&c->st_io, hipStreamDefault, least) != hipSuccess) { delete c; return LF_ERR_HIP; }
    (void)hipEventCreateWithFlags(&c->ev_block, hipEventBlockingSync | hipEventDisableTiming);
    u64 nr, y[24];
    default_ring(&nr, y);
    int rc = install_tables(c, nr, y);
    if (rc != LF_OK) { delete c; return rc; }
    *out = c;
    return LF_OK;
}
static void planes_pool_drop(int device);
void lf_ctx_destroy(lf_ctx *c) {
    if (!c) return;
    while (c->io_jobs.load() > 0) std::this_thread::yield();   // ingestion workers still use the context (their handles may be finished later: lf_witness_job_finish needs no context)
    (void)hipSetDevice(c->device);
    planes_pool_drop(c->device);
    if (c->bb) { c->bb->destroy(); delete c; return; }
    (void)c->sync_lanes();
    if (c->st_io) (void)hipStreamSynchronize(c->st_io);
    for (int l = 0; l < LF_NLANES; l++)
        if (c->stage[l]) (void)hipHostFree(c->stage[l]);
    if (c->h_pin2) { (void)hipHostFree(c->h_pin2); c->h_pin2 = nullptr; }
    if (c->ev_block) (void)hipEventDestroy(c->ev_block);
    c->comm[0].destroy();
    c->comm[1].destroy();
    if (c->tail_mail) (void)hipHostFree(c->tail_mail);
    if (c->tail_counters) (void)hipFree(c->tail_counters);
    if (c->d_poseidon) (void)hipFree(c->d_poseidon);
    if (c->zk_i8.dev) (void)hipFree(c->zk_i8.dev);
    if (c->ev_theta) (void)hipEventDestroy(c->ev_theta);
    if (c->ev_aux) (void)hipEventDestroy(c->ev_aux);
    if (c->st_aux) (void)hipStreamDestroy(c->st_aux);
    if (c->h_aux) (void)hipHostFree(c->h_aux);
    for (int i = 0; i < 2; i++)
        if (c->bits_ev[i]) (void)hipEventDestroy(c->bits_ev[i]);
    c->release_core();   // buffers, matrix, constraint system, per-lane pinned memory, the event pool and the three lanes' streams
    delete c;
}
int lf_set_ring_tables(lf_ctx *c, uint64_t nonres, const uint64_t *y) {
    if (!c || !y) return LF_ERR_INVALID;
    if (c->bb) return c->bb->set_ring_tables(nonres, y);
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return install_tables(c, nonres, y);
}
int lf_get_ring_tables(lf_ctx *c, uint64_t *nonres, uint64_t *y) {
    if (!c || !nonres || !y) return LF_ERR_INVALID;
    if (c->bb) return c->bb->get_ring_tables(nonres, y);
    *nonres = c->ring.T.nu;
    for (int k = 0; k < 8; k++)
        for (int q = 0; q < 3; q++) y[3 * k + q] = c->ring.T.y[k].c[q];
    return LF_OK;
}
// ---- external coordinate basis: marshalling of one ABI call ---------------------------------------------------------
// With a non-identity basis every entry point below first re-enters itself on converted copies of its NTT-form inputs (external ->
// internal coordinates), converts its outputs back in place, and -- for the prover entry points -- switches the transcript into
// "absorb internal, speak external" mode for the duration of the call.

int lf_set_digit_mode(lf_ctx *c, int mode) {
    if (!c || (mode != 0 && mode != 1)) return LF_ERR_INVALID;
    std::lock_guard<std::mutex> g(c->mu);
    c->core_any().digit_mode = mode;
    return LF_OK;
}
int lf_set_ext_basis(lf_ctx *c, const uint64_t *T) {
    if (!c || !T) return LF_ERR_INVALID;
    std::lock_guard<std::mutex> g(c->mu);
    const int ring = lf_ctx_ring(c);
    ExtBasis nb = c->xb;
    RET(nb.set(T, lf_ring_tau(ring), lf_ring_modulus(ring)));   // (a refused matrix leaves the basis in force, on the host and on the device, as it was)
    c->xb = nb;
    // the copies the relayout kernels take, in the ring's device word form
    const int tt = nb.tau * nb.tau;
    if (c->bb) {
        lfbb::BbCtxImpl *b = c->bb->p;
        std::lock_guard<std::mutex> gb(b->mu);
        b->xb_on = nb.on;
        for (int i = 0; i < tt; i++) { b->xb_T[i] = lfbb::from_canon(nb.T[i]); b->xb_Ti[i] = lfbb::from_canon(nb.Ti[i]); }
    } else {
        c->xb_on = nb.on;
        for (int i = 0; i < tt; i++) { c->xb_T[i] = nb.T[i]; c->xb_Ti[i] = nb.Ti[i]; }
    }
    return LF_OK;
}
int lf_set_sharding(lf_ctx *c, int rank, int world, lf_exchange_fn cb, void *user) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world & (world - 1)) != 0 || (world > 1 && !cb)) return LF_ERR_INVALID;
    if (c->bb) return c->bb->set_sharding(rank, world, cb, user);
    std::lock_guard<std::mutex> g(c->mu);
    if (c->A_loaded) return LF_ERR_STATE;  // choose the sharding before loading/generating the Ajtai matrix
    for (int l = 0; l < 2; l++) {
        c->comm[l].destroy();
        c->comm[l].rank = rank; c->comm[l].world = world; c->comm[l].cb = cb; c->comm[l].user = user; c->comm[l].poisoned = false; c->comm[l].model = false;
    }
    c->sh_rank = rank; c->sh_world = world;
    c->two_lanes_ok = false;                 // one channel: one thread issues every exchange
    c->agreed_two_lanes = -1;
    return LF_OK;
}
// Timing model of ONE rank of a sharded run on a box with one GPU (tools/shard_model.py): rank `rank` of `world` with no peers.  Every kernel and every host
// stage does exactly the share of the work that rank would do, every exchange is enqueued in the lane's stream (the peers' words are zeros), the two-lane
// schedule is the one a passed lf_dist_init self-check selects.  What the step returns is NOT a proof (the peers' partial sums are missing).
int lf_set_sharding_model(lf_ctx *c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world & (world - 1)) != 0) return LF_ERR_INVALID;
    if (c->bb) return LF_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> g(c->mu);
    if (c->A_loaded) return LF_ERR_STATE;
    for (int l = 0; l < 2; l++) {
        c->comm[l].destroy();
        c->comm[l].rank = rank; c->comm[l].world = world; c->comm[l].cb = nullptr; c->comm[l].user = nullptr; c->comm[l].poisoned = false; c->comm[l].model = world > 1;
    }
    c->sh_rank = rank; c->sh_world = world;
    c->two_lanes_ok = world > 1;
    c->agreed_two_lanes = -1;
    return LF_OK;
}
int lf_dist_stats_words(lf_ctx *c, uint64_t *words_sent, int reset) {
    if (!c || !words_sent) return LF_ERR_INVALID;
    if (c->bb) { *words_sent = 0; return LF_OK; }
    *words_sent = c->comm[0].words_sent + c->comm[1].words_sent;
    if (reset) c->comm[0].words_sent = c->comm[1].words_sent = 0;
    return LF_OK;
}
// all-gather `words` canonical words from every rank and add them mod p (RCCL has no modular reduction): device buffer, ordered on the lane's stream (RCCL: no host synchronisation; the reduction is k_modsum)
int exchange_modsum_dev(lf_ctx *c, u64 *inout_dev, size_t words) {
    if (c->sh_world <= 1 && !(c->tn.force_exchange && c->cm().nccl)) return LF_OK;   // LF_DIST_FORCE_EXCHANGE: a 1-rank communicator still runs the collectives (RCCL plumbing test on one GPU)
    u64 *g;
    RET(c->tbuf("sh_gather", (size_t)c->sh_world * words, &g));
    RET(c->cm().allgather_dev(inout_dev, g, words, c->stream()));
    launch_modsum(g, (u32)c->sh_world, words, inout_dev, c->stream());
    return LF_OK;
}
int lf_dist_unique_id(uint8_t *id128) { return lfdist::rccl_unique_id(id128); }
// Start-up self-check of the two-lane schedule (lf_dist_init): the FIRST collectives of both communicators are issued concurrently by the two threads that issue
// them in a fold step -- lane 0 by the caller, lane 1 by the helper thread -- each on its lane's stream, four rounds of all-gathers with rank-, lane- and
// round-dependent words, and every word received is checked.  Passed: the step runs the threaded schedule (LF_SHARD_TWO_LANES unset).  Wrong words: the
// communicators stay usable and one host thread issues every exchange (the conservative schedule).  No completion within the time limit
// (LF_DIST_HANDSHAKE_MS, default 20 s): both communicators are aborted and LF_ERR_STATE is returned -- the launcher makes fresh ids and calls lf_dist_init
// again with LF_DIST_NO_HANDSHAKE=1 (latticefold_amd/dist.py does).
static int dist_handshake(lf_ctx *c) {
    c->two_lanes_ok = false;
    if (getenv("LF_DIST_NO_HANDSHAKE")) return LF_OK;
    const int W = c->sh_world, R = c->sh_rank, ITER = 4;
    const size_t words = 64, per_it = words * (size_t)(W + 1);
    const long limit_ms = 20000;
    u64 *dbuf[2] = {nullptr, nullptr}, *hbuf[2] = {nullptr, nullptr};
    for (int l = 0; l < 2; l++) {
        if (lf_dev_malloc(&dbuf[l], per_it * ITER * 8) != hipSuccess || hipHostMalloc((void **)&hbuf[l], per_it * ITER * 8) != hipSuccess) {
            for (int q = 0; q < 2; q++) { if (dbuf[q]) (void)hipFree(dbuf[q]); if (hbuf[q]) (void)hipHostFree(hbuf[q]); }
            return LF_ERR_HIP;
        }
    }
    auto word = [](int g, int lane, int it, size_t w) { return ((u64)(g + 1) * 0x9E3779B97F4A7C15ull) ^ ((u64)lane << 40) ^ ((u64)it << 32) ^ (u64)w; };
    auto run = [&](int lane) -> int {
        const int keep = t_lane;
        t_lane = lane;
        int rc = hipSetDevice(c->device) == hipSuccess ? LF_OK : LF_ERR_HIP;
        for (int it = 0; it < ITER && rc == LF_OK; it++) {
            u64 *hs = hbuf[lane] + per_it * it, *ds = dbuf[lane] + per_it * it;
            for (size_t w = 0; w < words; w++) hs[w] = word(R, lane, it, w);
            if (hipMemcpyAsync(ds, hs, words * 8, hipMemcpyHostToDevice, c->stream()) != hipSuccess) { rc = LF_ERR_HIP; break; }
            rc = c->cm().allgather_dev(ds, ds + words, words, c->stream());
            if (rc == LF_OK && hipMemcpyAsync(hs + words, ds + words, words * W * 8, hipMemcpyDeviceToHost, c->stream()) != hipSuccess) rc = LF_ERR_HIP;
        }
        t_lane = keep;
        return rc;
    };
    c->lane1.submit([&]() -> int { return run(1); });
    int rc = run(0);
    const int rc1 = c->lane1.wait();
    if (rc == LF_OK) rc = rc1;
    bool timed_out = false;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(limit_ms);
    for (int l = 0; l < 2 && rc == LF_OK && !timed_out; l++)
        for (;;) {
            const hipError_t q = hipStreamQuery(c->st_lane[l]);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) { rc = LF_ERR_HIP; break; }
            if (std::chrono::steady_clock::now() > deadline) { timed_out = true; break; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    if (timed_out || rc != LF_OK) {      // the collectives may never complete: tear the communicators down (the buffers stay allocated -- a kernel may still hold them)
        c->comm[0].abort_peers(); c->comm[1].abort_peers();
        return LF_ERR_STATE;
    }
    bool ok = true;
    for (int l = 0; l < 2 && ok; l++)
        for (int it = 0; it < ITER && ok; it++)
            for (int g2 = 0; g2 < W && ok; g2++)
                for (size_t w = 0; w < words && ok; w++) ok = hbuf[l][per_it * it + words + (size_t)g2 * words + w] == word(g2, l, it, w);
    // The ranks must AGREE on the schedule: the threaded one splits the exchanges of a step over comm[0] and comm[1], the one-thread schedule issues all of them
    // on comm[0] -- ranks that chose differently would issue different collective sequences and hang.  So the verdict is exchanged inside the library (one more
    // all-gather on comm[0], one issuing thread: the form that works whatever the check found) and the minimum wins; a rank's own LF_SHARD_TWO_LANES=0 / =1 enters
    // it too (2 = forced on, 1 = check passed, 0 = off / failed: forced-on survives only if every rank forced it), so a C or Rust caller of lf_dist_init needs no
    // agreement of its own (the Python launcher's MIN-reduce is no longer what correctness rests on).
    {
        const char *e = getenv("LF_SHARD_TWO_LANES");
        const u64 mine = e ? (atoi(e) != 0 ? 2 : 0) : (ok ? 1 : 0);
        u64 *hs = hbuf[0], *ds = dbuf[0];
        hs[0] = mine;
        const int keep = t_lane;
        t_lane = 0;
        int rc2 = hipMemcpyAsync(ds, hs, 8, hipMemcpyHostToDevice, c->stream()) == hipSuccess ? LF_OK : LF_ERR_HIP;
        if (rc2 == LF_OK) rc2 = c->cm().allgather_dev(ds, ds + 1, 1, c->stream());
        if (rc2 == LF_OK && hipMemcpyAsync(hs + 1, ds + 1, (size_t)W * 8, hipMemcpyDeviceToHost, c->stream()) != hipSuccess) rc2 = LF_ERR_HIP;
        bool late = false;
        for (; rc2 == LF_OK;) {
            const hipError_t q = hipStreamQuery(c->stream());
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) { rc2 = LF_ERR_HIP; break; }
            if (std::chrono::steady_clock::now() > deadline) { late = true; break; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        t_lane = keep;
        if (late || rc2 != LF_OK) { c->comm[0].abort_peers(); c->comm[1].abort_peers(); return LF_ERR_STATE; }
        u64 mn = 2;
        for (int g2 = 0; g2 < W; g2++) mn = hs[1 + g2] < mn ? hs[1 + g2] : mn;
        ok = mn >= 1;                                          // every rank either passed the check or forces the threaded schedule
        c->agreed_two_lanes = ok ? 1 : 0;                      // what the sharded step follows (lf_fold_step), whatever this rank's environment says later
    }
    for (int l = 0; l < 2; l++) { (void)hipFree(dbuf[l]); (void)hipHostFree(hbuf[l]); c->comm[l].n_exchanges = 0; c->comm[l].us_total = 0; c->comm[l].us_max = 0; }
    c->two_lanes_ok = ok;
    return LF_OK;
}
int lf_dist_init(lf_ctx *c, int rank, int world, const uint8_t *ids) {
    if (!c || !ids || world < 1 || rank < 0 || rank >= world || (world & (world - 1)) != 0) return LF_ERR_INVALID;
    if (c->bb) return c->bb->dist_init(rank, world, ids);
    std::lock_guard<std::mutex> g(c->mu);
    if (c->A_loaded) return LF_ERR_STATE;   // choose the sharding before loading/generating the Ajtai matrix
    HIPCHK(hipSetDevice(c->device));
    for (int l = 0; l < 2; l++) {
        c->comm[l].destroy();
        RET(lfdist::rccl_init(c->comm[l], rank, world, ids + 128 * l));
    }
    c->sh_rank = rank; c->sh_world = world;
    return dist_handshake(c);
}
int lf_dist_two_lanes(lf_ctx *c, int set) {
    if (!c) return LF_ERR_INVALID;
    if (c->bb) return 0;                      // (the BabyBear driver exchanges from one thread only)
    std::lock_guard<std::mutex> g(c->mu);
    if (set == 0 || set == 1) { c->two_lanes_ok = set == 1; c->agreed_two_lanes = set; }   // (the caller sets the same value on every rank)
    return c->two_lanes_ok ? 1 : 0;
}
// per-lane callbacks (host transport): the two lanes of a fold step exchange concurrently, so each needs its own ordered channel
int lf_set_sharding_lanes(lf_ctx *c, int rank, int world, lf_exchange_fn cb0, void *user0, lf_exchange_fn cb1, void *user1) {
    int rc = lf_set_sharding(c, rank, world, cb0, user0);
    if (rc != LF_OK || !cb1) return rc;
    if (c->bb) return LF_OK;   // the BabyBear driver exchanges from one thread only
    std::lock_guard<std::mutex> g(c->mu);
    c->comm[1].cb = cb1; c->comm[1].user = user1;
    c->agreed_two_lanes = -1;
    c->two_lanes_ok = (cb1 != cb0 || user1 != user0);   // two ordered channels supplied by the host language: the threaded schedule is the default
    return LF_OK;
}
int lf_dist_stats(lf_ctx *c, uint64_t *n_exchanges, double *total_us, double *max_us, int reset) {
    if (!c) return LF_ERR_INVALID;
    lfdist::Comm *ms[2] = {c->bb ? &c->bb->p->comm : &c->comm[0], c->bb ? nullptr : &c->comm[1]};
    uint64_t n = 0;
    double tot = 0, mx = 0;
    for (auto *m : ms)
        if (m) {
            n += m->n_exchanges; tot += m->us_total; mx = m->us_max > mx ? m->us_max : mx;
            if (reset) { m->n_exchanges = 0; m->us_total = 0; m->us_max = 0; }
        }
    if (n_exchanges) *n_exchanges = n;
    if (total_us) *total_us = tot;
    if (max_us) *max_us = mx;
    return LF_OK;
}
int lf_mem_info(lf_ctx *c, size_t *free_bytes, size_t *total_bytes) {
    if (!c || !free_bytes || !total_bytes) return LF_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemGetInfo(free_bytes, total_bytes));
    return LF_OK;
}
int lf_device_synchronize(lf_ctx *c) {
    if (!c) return LF_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    if (c->bb) return c->bb->p->sync_lanes();
    HIPCHK(hipStreamSynchronize(c->stream()));
    return LF_OK;
}

// ---- host<->device staging (up_ring / down_ring: lf_ring_host.h) -----------------------------------------------
// small device array -> host (through pinned memory)
int down_small(lf_ctx *c, const u64 *dsrc, size_t words, u64 *host) {
    RET(c->pin(words));
    HIPCHK(hipMemcpyAsync(c->h_pin_ref(), dsrc, words * 8, hipMemcpyDeviceToHost, c->stream()));
    RET(c->lane_sync());
    memcpy(host, c->h_pin_ref(), words * 8);
    return LF_OK;
}
Fq3Const f3c(Fq3 a) { Fq3Const r; r.c[0] = a.c[0]; r.c[1] = a.c[1]; r.c[2] = a.c[2]; return r; }

// ---- arithmetic self-test -----------------------------------------------------------------------------------------
// The device computes (k_selftest_field), the host judges: every stored word is compared with `unsigned __int128 %` arithmetic written out here -- nothing of
// lf_field.cuh, whose host and device paths share their formulas.  The first operand pairs put every pair of the reduction-corner grid into every coordinate
// position (the borrow / carry / hl == 0 branches of fq_reduce128_loose, both wraps of fq_from_s128 and results in [p, 2^64) occur only there: uniform words
// never reach them); the rest are pseudo-random from `seed` with a quarter of the words drawn from the grid.
namespace selftest {
typedef unsigned __int128 u128;
constexpr u64 PM = 0xFFFFFFFF00000001ULL;
constexpr int NG = 22;
const u64 GRID[NG] = {0, 1, 2, PM - 1, PM - 2, 0xFFFFFFFFULL, 1ULL << 32, (1ULL << 32) + 1, (1ULL << 32) + 2, PM - 0xFFFFFFFFULL, 0xFFFFFFFEULL,
                      (PM - 1) / 2, (PM + 1) / 2, 1ULL << 63, (1ULL << 63) + 1, 1ULL << 40, 1ULL << 24, PM - (1ULL << 40), 0xFFFFFFFE00000001ULL,
                      3ULL << 62, 0x1FFFFFFFFULL, PM - (1ULL << 24)};
inline u64 md(u128 v) { return (u64)(v % PM); }
inline u64 mm(u64 a, u64 b) { return md((u128)a * b); }
struct E3 { u64 c[3]; };
inline void columns(const E3 &a, const E3 &b, u64 col[5]) {   // the five schoolbook column sums, each reduced
    col[0] = mm(a.c[0], b.c[0]);
    col[1] = md((u128)mm(a.c[0], b.c[1]) + mm(a.c[1], b.c[0]));
    col[2] = md((u128)mm(a.c[0], b.c[2]) + mm(a.c[1], b.c[1]) + mm(a.c[2], b.c[0]));
    col[3] = md((u128)mm(a.c[1], b.c[2]) + mm(a.c[2], b.c[1]));
    col[4] = mm(a.c[2], b.c[2]);
}
inline E3 finish(const u64 col[5], u64 nu) {                  // Y^3 = nu
    E3 r;
    r.c[0] = md((u128)col[0] + mm(nu, col[3]));
    r.c[1] = md((u128)col[1] + mm(nu, col[4]));
    r.c[2] = col[2];
    return r;
}
inline unsigned differ(const u64 *got, const E3 &want) { return (got[0] != want.c[0]) + (got[1] != want.c[1]) + (got[2] != want.c[2]); }
void operands(u64 seed, u32 n, std::vector<u64> &in) {
    in.resize((size_t)n * 6);
    u32 i = 0;
    for (int sh = 0; sh < 3 && i < n; sh++)
        for (int x = 0; x < NG && i < n; x++)
            for (int y = 0; y < NG && i < n; y++, i++) {
                u64 *w = &in[(size_t)i * 6];
                w[0] = GRID[x]; w[1] = GRID[(x + sh) % NG]; w[2] = GRID[(x + 2 * sh) % NG];
                w[3] = GRID[y]; w[4] = GRID[(y + 5 * sh) % NG]; w[5] = GRID[(y + 7 * sh) % NG];
            }
    u64 s = seed * 0x9E3779B97F4A7C15ULL + 1;
    for (size_t k = (size_t)i * 6; k < in.size(); k++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        in[k] = ((s >> 7) & 3) == 0 ? GRID[(s >> 11) % NG] : s % PM;
    }
}
// mismatching words among the outputs of operand pairs [i0, i1)
u64 check(const u64 *in, const u64 *out, const u64 *outc, u32 nc, u64 nu_gen, u32 i0, u32 i1) {
    const u64 nu = 1ULL << 40;
    u64 bad = 0;
    for (u32 i = i0; i < i1; i++) {
        const u64 *w = in + (size_t)i * 6, *o = out + (size_t)i * SELFTEST_OUT;
        E3 a = {{w[0], w[1], w[2]}}, b = {{w[3], w[4], w[5]}};
        bad += o[0] != md((u128)a.c[0] + b.c[0]);
        bad += o[1] != md((u128)a.c[0] + PM - b.c[0]);
        bad += o[2] != mm(a.c[0], b.c[0]);
        bad += o[3] != mm(a.c[0], nu);
        u64 col[5];
        columns(a, b, col);
        const E3 p40 = finish(col, nu);
        bad += differ(o + 4, p40) + differ(o + 7, p40) + differ(o + 10, finish(col, nu_gen));
        if (i < nc) {
            E3 x = a, y = b, sum = {{0, 0, 0}};
            for (int r = 0; r < 37; r++) {
                columns(x, y, col);
                const E3 pr = finish(col, nu);
                E3 t;
                for (int q = 0; q < 3; q++) { sum.c[q] = md((u128)sum.c[q] + pr.c[q]); t.c[q] = md((u128)x.c[q] + y.c[q]); }
                x = y; y = t;
            }
            const u64 *oc = outc + (size_t)i * SELFTEST_OUTC;
            bad += differ(oc, sum) + differ(oc + 3, sum) + differ(oc + 6, sum) + differ(oc + 9, sum);
        }
    }
    return bad;
}
}  // namespace selftest

int lf_selftest_field(lf_ctx *c, uint64_t seed, uint32_t n, uint64_t *mismatches) {
    if (!c || !mismatches) return LF_ERR_INVALID;
    if (c->bb) return c->bb->selftest_field(seed, n, mismatches);
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    const u32 nc = n < (1u << 14) ? n : (1u << 14);     // the 37-term sums are checked on the grid pairs and the first pseudo-random ones (37 products each on the host)
    const u64 nu_gen = c->dcrt.nu2p40 ? 0xFFFFFFFE00000002ULL : c->dcrt.nu;   // the context's own non-residue where it is not 2^40
    std::vector<u64> in, out((size_t)n * SELFTEST_OUT), outc((size_t)nc * SELFTEST_OUTC);
    selftest::operands(seed, n, in);
    u64 *d, *di, *dout, *doutc;
    RET(c->tbuf("small_dev", 4096, &d));
    RET(c->tbuf("io_a", in.size() + 8, &di));
    RET(c->tbuf("io_b", out.size() + 8, &dout));
    RET(c->tbuf("io_c", outc.size() + 8, &doutc));
    u64 dev_bad = 0;
    if (n) {
        HIPCHK(hipMemcpyAsync(di, in.data(), in.size() * 8, hipMemcpyHostToDevice, c->stream()));
        launch_selftest_field(di, n, nc, nu_gen, dout, doutc, d, c->stream());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost, c->stream()));
        HIPCHK(hipMemcpyAsync(outc.data(), doutc, outc.size() * 8, hipMemcpyDeviceToHost, c->stream()));
        HIPCHK(hipMemcpyAsync(&dev_bad, d, 8, hipMemcpyDeviceToHost, c->stream()));
        HIPCHK(hipStreamSynchronize(c->stream()));
    }
    // the pairs with 37-term sums cost most: they go round-robin in blocks of 256 pairs over the checking threads
    const u32 nthr = n >= (1u << 14) ? 8 : 1;
    const u64 blocks = ((u64)n + 255) / 256;      // (64-bit: n within 255 of 2^32 must not wrap)
    std::vector<u64> bad(nthr, 0);
    std::vector<std::thread> th;
    auto work = [&](u32 t) {
        for (u64 bl = t; bl < blocks; bl += nthr) {
            const u64 i0 = bl * 256, i1 = i0 + 256 < n ? i0 + 256 : n;
            bad[t] += selftest::check(in.data(), out.data(), outc.data(), nc, nu_gen, (u32)i0, (u32)i1);
        }
    };
    for (u32 t = 1; t < nthr; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    u64 total = dev_bad;
    for (u64 v : bad) total += v;
    *mismatches = total;
    return LF_OK;
}

// ---- a1/a2 --------------------------------------------------------------------------------------------------------
int lf_ntt_fwd(lf_ctx *c, const uint64_t *in, uint64_t *out, size_t count) {
    XbArrays xa(c);
    if (!c || (!in && count) || (!out && count)) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::ntt_fwd(c->bb->p, in, out, count) : ring_ops<GoldRing>::ntt_fwd(c, in, out, count);
}
int lf_ntt_inv(lf_ctx *c, const uint64_t *in, uint64_t *out, size_t count) {
    XbArrays xa(c);
    if (!c || (!in && count) || (!out && count)) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::ntt_inv(c->bb->p, in, out, count) : ring_ops<GoldRing>::ntt_inv(c, in, out, count);
}
// ---- the _dev twins (include/lfhip.h "device-resident callers"): the same bodies with Origin::device.  Here: the null checks of the host twin; on a context in
// an external basis the caller's array is read and written in external coordinates, like the host twin's (XbArrays: the relayout kernels convert).  The pointer
// checks proper -- dev_array_check, lf_ring_host.h -- run inside the body, after its state and length checks and before its first launch
// in and out of `words` words each: the same array or disjoint ones
static bool same_or_disjoint(const uint64_t *in, const uint64_t *out, size_t words) { return in == out || in + words <= out || out + words <= in; }
int lf_ntt_fwd_dev(lf_ctx *c, const uint64_t *in, uint64_t *out, size_t count) {
    if (!c || (!in && count) || (!out && count) || !same_or_disjoint(in, out, count * lf_ring_words(lf_ctx_ring(c)))) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::ntt_fwd(c->bb->p, in, out, count, Origin::device) : ring_ops<GoldRing>::ntt_fwd(c, in, out, count, Origin::device);
}
int lf_ntt_inv_dev(lf_ctx *c, const uint64_t *in, uint64_t *out, size_t count) {
    if (!c || (!in && count) || (!out && count) || !same_or_disjoint(in, out, count * lf_ring_words(lf_ctx_ring(c)))) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::ntt_inv(c->bb->p, in, out, count, Origin::device) : ring_ops<GoldRing>::ntt_inv(c, in, out, count, Origin::device);
}
// the ring as a ring: sum of n_terms products of arrays, NTT form (slot-wise) or coefficient form (transforms fused); one body for both spellings and both rings
static int ring_mul_api(lf_ctx *c, const uint64_t *a, const uint64_t *b, size_t n_terms, size_t count, int form, uint64_t *out, Origin org) {
    if (!c || !a || !b || !out || !n_terms || (form != LF_FORM_NTT && form != LF_FORM_COEFF)) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::ring_mul(c->bb->p, a, b, n_terms, count, form, out, org) : ring_ops<GoldRing>::ring_mul(c, a, b, n_terms, count, form, out, org);
}
int lf_ring_mul(lf_ctx *c, const uint64_t *a, const uint64_t *b, size_t n_terms, size_t count, int form, uint64_t *out) {
    return ring_mul_api(c, a, b, n_terms, count, form, out, Origin::host);
}
int lf_ring_mul_device(lf_ctx *c, const uint64_t *a, const uint64_t *b, size_t n_terms, size_t count, int form, uint64_t *out) {
    return ring_mul_api(c, a, b, n_terms, count, form, out, Origin::device);
}
// Order the context's lanes behind the work enqueued so far on a stream of the caller's: an event recorded there, waited for by every lane.  The host does not
// wait and the caller's stream is not touched otherwise
int lf_ctx_wait_stream(lf_ctx *c, void *hip_stream) {
    if (!c) return LF_ERR_INVALID;
    CtxCoreBase &k = c->core_any();
    std::lock_guard<std::mutex> g(k.mu);
    HIPCHK(hipSetDevice(c->device));
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, (hipStream_t)hip_stream);
    for (int l = 0; l < LF_NLANES && e == hipSuccess; l++)
        if (k.st_lane[l]) e = hipStreamWaitEvent(k.st_lane[l], ev, 0);
    (void)hipEventDestroy(ev);   // (released by the runtime once the waits have passed)
    return e == hipSuccess ? LF_OK : LF_ERR_HIP;
}
int lf_decompose(lf_ctx *c, const uint64_t *in, size_t count, uint64_t base, unsigned digits, int layout, uint64_t *out) {
    if (!c || !in || !out || digits == 0 || digits > 64 || (layout != 0 && layout != 1)) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::decompose(c->bb->p, in, count, base, digits, layout, out) : ring_ops<GoldRing>::decompose(c, in, count, base, digits, layout, out);
}
int lf_recompose(lf_ctx *c, const uint64_t *in, size_t count_out, uint64_t base, unsigned digits, uint64_t *out) {
    if (!c || !in || !out || digits == 0) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::recompose(c->bb->p, in, count_out, base, digits, out) : ring_ops<GoldRing>::recompose(c, in, count_out, base, digits, out);
}
int lf_linf_check(lf_ctx *c, const uint64_t *f_ntt, size_t count, uint64_t bound, int unsigned_variant, int *ok, uint64_t *max_out) {
    XbArrays xa(c);
    if (!c || !f_ntt || !ok) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::linf_check(c->bb->p, f_ntt, count, bound, unsigned_variant, ok, max_out) : ring_ops<GoldRing>::linf_check(c, f_ntt, count, bound, unsigned_variant, ok, max_out);
}
// (coefficient-form arrays: no basis, so no XbArrays; the overlap of `in` and `out` is refused in the body, behind its state checks)
int lf_decompose_dev(lf_ctx *c, const uint64_t *in, size_t count, uint64_t base, unsigned digits, int layout, uint64_t *out) {
    if (!c || !in || !out || digits == 0 || digits > 64 || (layout != 0 && layout != 1)) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::decompose(c->bb->p, in, count, base, digits, layout, out, Origin::device)
                 : ring_ops<GoldRing>::decompose(c, in, count, base, digits, layout, out, Origin::device);
}
int lf_recompose_dev(lf_ctx *c, const uint64_t *in, size_t count_out, uint64_t base, unsigned digits, uint64_t *out) {
    if (!c || !in || !out || digits == 0) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::recompose(c->bb->p, in, count_out, base, digits, out, Origin::device)
                 : ring_ops<GoldRing>::recompose(c, in, count_out, base, digits, out, Origin::device);
}
int lf_linf_check_dev(lf_ctx *c, const uint64_t *f_ntt, size_t count, uint64_t bound, int unsigned_variant, int *ok, uint64_t *max_out) {
    if (!c || !f_ntt || !ok) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::linf_check(c->bb->p, f_ntt, count, bound, unsigned_variant, ok, max_out, Origin::device)
                 : ring_ops<GoldRing>::linf_check(c, f_ntt, count, bound, unsigned_variant, ok, max_out, Origin::device);
}

// ---- a5 -----------------------------------------------------------------------------------------------------------
int lf_ajtai_load(lf_ctx *c, const uint64_t *A, size_t kappa, size_t n) {
    XbArrays xa(c);
    if (!c || !A || !kappa || !n || kappa > 128) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::ajtai_install(c->bb->p, kappa, n, A, 0) : ring_ops<GoldRing>::ajtai_install(c, kappa, n, A, 0);
}
int lf_ajtai_generate(lf_ctx *c, uint64_t seed, size_t kappa, size_t n) {
    if (!c || !kappa || !n || kappa > 128) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::ajtai_install(c->bb->p, kappa, n, nullptr, seed) : ring_ops<GoldRing>::ajtai_install(c, kappa, n, nullptr, seed);
}
int lf_device_memory(lf_ctx *c, size_t *free_bytes, size_t *total_bytes) {
    if (!c || !free_bytes || !total_bytes) return LF_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemGetInfo(free_bytes, total_bytes));
    return LF_OK;
}
// The K - 1 part commitments of a base-b decomposition (decomposition.rs:178-201) as the planes of ONE general-commit launch per row chunk: A leaves HBM once
// per decomposition.  D [NP][24][ldn] are the operand words already (lf_sb.h); the finish writes every plane's commitment instead of recombining them.
int commit_parts_i8g(lf_ctx *c, const unsigned char *D, size_t ldn, u32 NP, u64 *out_dev) {
    if (!c->A_loaded || !c->i8_nch || !c->dAb) return LF_ERR_STATE;
    if (c->A_col0 != 0 || c->nA != c->N || ldn != sb_ld(c->N)) return LF_ERR_UNSUPPORTED;
    const AjtaiI8Ring R = ajtai_i8_goldilocks();
    const u32 nch = c->i8_nch, kc = c->i8_kc, MT = ajtai_i8_row_tiles(R, kc), nwg = 256;
    const size_t ntiles = (c->nA + 7) / 8, chunk_bytes = ntiles * (R.RD / 8) * MT * 1024;
    size_t pw, dw, sw;
    if (ajtai_i8g_scratch(R, MT, c->nA, NP, nwg, &pw, &dw, &sw) != 0) return LF_ERR_UNSUPPORTED;
    int32_t *part, *dsum;
    long long *sum;
    u64 *coef, *ntt;
    const size_t ne = (size_t)NP * c->kappa;
    RET(c->tbuf("i8g_part", pw, &part));
    RET(c->tbuf("i8g_dsum", dw, &dsum));
    RET(c->tbuf("i8g_sum", sw, &sum));
    RET(c->tbuf("sb_y_coef", 24 * ne, &coef));
    RET(c->tbuf("sb_y_ntt", 24 * ne, &ntt));
    const size_t ev = c->ev_begin(1);
    for (u32 ch = 0; ch < nch; ch++) {
        const u32 row0 = ch * kc, kn = c->kappa - row0 < kc ? c->kappa - row0 : kc;
        const int g = launch_ajtai_i8g(R, c->dAb + (size_t)ch * chunk_bytes, MT, (const unsigned long long *)D, ldn / 8, c->nA, kn, row0, c->kappa, NP, nwg, part, dsum, sum,
                                       coef, c->stream(), 1, c->tn.i8g_prof);
        if (g < 0) return i8_rc(g);
    }
    c->ev_end(ev);
    launch_crt_fwd(c->dcrt, coef, ntt, ne, c->stream());
    launch_soa_to_aos(ntt, out_dev, ne, c->stream());
    if (hipGetLastError() != hipSuccess) return LF_ERR_HIP;
    return LF_OK;
}
int sb_cut_parts(lf_ctx *c, const lf_witness *wit, const char *name, const unsigned char **D) {
    const lf_params &P = c->P;
    if (!sb_base_ok(P.b) || c->sh_world > 1 || c->comm[0].model) return LF_ERR_UNSUPPORTED;
    if (!sb_digits_cover(P.b, P.K, P.B, c->digit_mode)) return LF_ERR_UNSUPPORTED;   // never a truncated decomposition
    unsigned char *d;
    const size_t ldn = sb_ld(c->N);
    RET(c->tbuf(name, (size_t)P.K * 24 * ldn, &d));
    if (launch_sb_cut(wit->planes, c->N, P.K, sb_log2(P.b), c->digit_mode, d, ldn, c->stream()) != 0) return LF_ERR_HIP;
    *D = d;
    return LF_OK;
}
// download a (partial) commitment and, when sharded, all-gather + add the partials mod p
int commit_download(lf_ctx *c, const u64 *dev, size_t words, u64 *host) {
    RET(exchange_modsum_dev(c, (u64 *)dev, words));   // sharded: ncclAllGather of the partial commitments + k_modsum, in stream
    return down_small(c, dev, words, host);
}
// index slice of this rank: [*i0, *i0 + *cnt) of n items (the last rank takes the remainder)
void shard_slice(const lf_ctx *c, size_t n, size_t *i0, size_t *cnt) {
    size_t per = (n + (size_t)c->sh_world - 1) / (size_t)c->sh_world;
    size_t lo = per * (size_t)c->sh_rank;
    if (lo > n) lo = n;
    *i0 = lo;
    *cnt = lo + per > n ? n - lo : per;
}
// Sharded sumchecks: tables of `n` entries stay sharded while every rank keeps at least 64 pairs AND the tables are larger than the hand-over size of the
// sumcheck (kind 0 linearization, 1 folding; Tunables::shard_lin_min / shard_fold_min, never above m / 16 so that small instances still exercise the sharded
// rounds).  Every rank evaluates the same predicate on the same numbers: the ranks leave the sharded form in the same round.
bool shard_keep(const lf_ctx *c, int kind, size_t n) {
    const size_t Gw = (size_t)c->sh_world;
    if (Gw <= 1 || n / 2 < Gw * 64) return false;
    size_t thr = kind ? c->tn.shard_fold_min : c->tn.shard_lin_min;
    if (thr > (c->m >> 4)) thr = c->m >> 4;
    return n > thr;
}
// all-gather the ranks' column slices of `planes` tables stored with GLOBAL layout [plane][n] (rank g holds entries
// [g*n/G, (g+1)*n/G) of every plane) and fill in the others' slices
int gather_slices(lf_ctx *c, u64 *buf, size_t planes, size_t n) {
    const size_t Gw = (size_t)c->sh_world, lcl = n / Gw, words = planes * lcl;
    u64 *gall, *gtmp;
    RET(c->tbuf("sh_gather_tab", words * Gw, &gall));
    RET(c->tbuf("sh_gather_tmp", words, &gtmp));
    HIPCHK(hipMemcpy2DAsync(gtmp, lcl * 8, buf + (size_t)c->sh_rank * lcl, n * 8, lcl * 8, planes, hipMemcpyDeviceToDevice, c->stream()));
    RET(c->cm().allgather_dev(gtmp, gall, words, c->stream()));
    launch_gather_relayout(gall, (u32)Gw, planes, lcl, buf, c->stream());
    return LF_OK;
}
// Several table sets in ONE exchange (the hand-over of a sharded sumcheck to its replicated rounds): part i is this rank's `lcl` entries of `planes` rows
// at src (row stride src_ld) and becomes the full tables dst [planes][G lcl] on every rank.  src may lie inside dst (the payload is staged first).
int gather_parts(lf_ctx *c, const GatherPart *parts, int np, size_t lcl) {
    const size_t Gw = (size_t)c->sh_world;
    size_t ptot = 0;
    for (int i = 0; i < np; i++) ptot += parts[i].planes;
    const size_t words = ptot * lcl;
    u64 *gall, *gtmp;
    RET(c->tbuf("sh_gather_tab", words * Gw, &gall));
    RET(c->tbuf("sh_gather_tmp", words, &gtmp));
    size_t p0 = 0;
    for (int i = 0; i < np; i++) {
        HIPCHK(hipMemcpy2DAsync(gtmp + p0 * lcl, lcl * 8, parts[i].src, parts[i].src_ld * 8, lcl * 8, parts[i].planes, hipMemcpyDeviceToDevice, c->stream()));
        p0 += parts[i].planes;
    }
    RET(c->cm().allgather_dev(gtmp, gall, words, c->stream()));
    p0 = 0;
    for (int i = 0; i < np; i++) {
        launch_gather_relayout_part(gall, (u32)Gw, ptot, p0, parts[i].planes, lcl, parts[i].dst, c->stream());
        p0 += parts[i].planes;
    }
    return LF_OK;
}
int lf_ajtai_commit(lf_ctx *c, const uint64_t *f, size_t n, size_t batch, uint64_t *out) {
    if (LF_XB(c) && f && out) {
        XB x(c, true);   // f changes basis on the device; the commitments are small: on the host
        int rc = lf_ajtai_commit(c, f, n, batch, out);
        if (rc == LF_OK) x.ring_out(out, batch * c->core_any().kappa);
        return rc;
    }
    if (!c || !f || !out || !batch) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::ajtai_commit(c->bb->p, f, n, batch, out) : ring_ops<GoldRing>::ajtai_commit(c, f, n, batch, out);
}
int lf_ajtai_commit_dev(lf_ctx *c, const uint64_t *f, size_t n, size_t batch, uint64_t *out) {
    if (!c || !f || !out || !batch) return LF_ERR_INVALID;
    if (LF_XB(c)) {
        XB x(c, true);
        int rc = lf_ajtai_commit_dev(c, f, n, batch, out);
        if (rc == LF_OK) x.ring_out(out, batch * c->core_any().kappa);
        return rc;
    }
    return c->bb ? ring_ops<BbRing>::ajtai_commit(c->bb->p, f, n, batch, out, Origin::device) : ring_ops<GoldRing>::ajtai_commit(c, f, n, batch, out, Origin::device);
}
// The ABI side of the three (dec false: commit_coeff, no decomposition): arguments are checked before any device work; in an external basis the commitments
// leave converted and NTT-form input is converted on the way in, coefficient-form input is not (as lf_witness_from_f_coeff).
static int ajtai_commit_gadget_api(lf_ctx *c, const uint64_t *f, bool ntt_in, size_t count, bool dec, uint64_t base, unsigned digits, size_t batch, uint64_t *out,
                                   Origin org = Origin::host) {
    if (LF_XB(c) && f && out) {
        XB x(c, true);   // (the body stages NTT-form input as Form::ntt, coefficient-form input as Form::coeff)
        const u32 kap = c->core_any().kappa;
        int rc = ajtai_commit_gadget_api(c, f, ntt_in, count, dec, base, digits, batch, out, org);
        if (rc == LF_OK) x.ring_out(out, batch * kap);
        return rc;
    }
    if (!c || !f || !out || !batch || digits == 0 || digits > 64) return LF_ERR_INVALID;
    u32 lb = 0;
    if (dec) {
        if (!pow2(base) || (c->bb && base > (1ull << 32))) return LF_ERR_UNSUPPORTED;
        while ((1ull << lb) < base) lb++;
    }
    return c->bb ? ring_ops<BbRing>::ajtai_commit_gadget(c->bb->p, f, ntt_in, count, lb, digits, batch, out, org)
                 : ring_ops<GoldRing>::ajtai_commit_gadget(c, f, ntt_in, count, lb, digits, batch, out, org);
}
int lf_ajtai_commit_coeff(lf_ctx *c, const uint64_t *f_coeff, size_t n, size_t batch, uint64_t *out) {
    return ajtai_commit_gadget_api(c, f_coeff, false, n, false, 0, 1, batch, out);
}
int lf_ajtai_decompose_and_commit_coeff(lf_ctx *c, const uint64_t *f_coeff, size_t count, uint64_t base, unsigned digits, size_t batch, uint64_t *out) {
    return ajtai_commit_gadget_api(c, f_coeff, false, count, true, base, digits, batch, out);
}
int lf_ajtai_decompose_and_commit_ntt(lf_ctx *c, const uint64_t *w_ntt, size_t count, uint64_t base, unsigned digits, size_t batch, uint64_t *out) {
    return ajtai_commit_gadget_api(c, w_ntt, true, count, true, base, digits, batch, out);
}
int lf_ajtai_commit_coeff_dev(lf_ctx *c, const uint64_t *f_coeff, size_t n, size_t batch, uint64_t *out) {
    return ajtai_commit_gadget_api(c, f_coeff, false, n, false, 0, 1, batch, out, Origin::device);
}
int lf_ajtai_decompose_and_commit_coeff_dev(lf_ctx *c, const uint64_t *f_coeff, size_t count, uint64_t base, unsigned digits, size_t batch, uint64_t *out) {
    return ajtai_commit_gadget_api(c, f_coeff, false, count, true, base, digits, batch, out, Origin::device);
}
int lf_ajtai_decompose_and_commit_ntt_dev(lf_ctx *c, const uint64_t *w_ntt, size_t count, uint64_t base, unsigned digits, size_t batch, uint64_t *out) {
    return ajtai_commit_gadget_api(c, w_ntt, true, count, true, base, digits, batch, out, Origin::device);
}

// column-sharded commit: the context holds only columns [col0, col0+n_local) of A (loaded with lf_ajtai_load on
// that slice); f is the matching slice of each witness.  The result is the PARTIAL commitment of this shard; the caller
// exchanges partials (all-gather) and adds them mod p -- lf_modsum -- because RCCL has no modular reduction.
int lf_modsum(const uint64_t *parts, size_t nparts, size_t words, uint64_t *out) {
    if (!parts || !out || !nparts) return LF_ERR_INVALID;
    for (size_t w = 0; w < words; w++) {
        u64 acc = 0;
        for (size_t g = 0; g < nparts; g++) {
            u64 v = parts[g * words + w];
            if (v >= LF_P) return LF_ERR_INVALID;
            acc = fq_add(acc, v);
        }
        out[w] = acc;
    }
    return LF_OK;
}
int lf_modsum_ring(const uint64_t *parts, size_t nparts, size_t words, uint64_t *out, int ring) {
    if (ring == LF_RING_GOLDILOCKS) return lf_modsum(parts, nparts, words, out);
    if (ring != LF_RING_BABYBEAR || !parts || !out || !nparts) return LF_ERR_INVALID;
    for (size_t w = 0; w < words; w++) {
        u64 acc = 0;
        for (size_t g = 0; g < nparts; g++) {
            u64 v = parts[g * words + w];
            if (v >= lfbb::BB_P) return LF_ERR_INVALID;
            acc += v;                         // nparts * p < 2^64 for any realistic rank count
        }
        out[w] = acc % lfbb::BB_P;
    }
    return LF_OK;
}

// ---- a8/a9/a11 ------------------------------------------------------------------------------------------------------
int build_eq_dev(lf_ctx *c, const Fq3 *pt, u32 nv, u64 *eq_dev) {
    Fq3Const *rd;
    RET(c->tbuf("eq_point", 64, &rd));
    std::vector<Fq3Const> h(nv);
    for (u32 i = 0; i < nv; i++) h[i] = f3c(pt[i]);
    RET(c->h2d_small(rd, h.data(), nv * sizeof(Fq3Const)));
    if (nv >= 6) {   // two-level: one product per entry
        u64 *scr;
        RET(c->tbuf("eq_scratch", build_eq_scratch_words(nv), &scr));
        launch_build_eq2(c->dcrt, rd, nv, scr, eq_dev, c->stream());
    } else launch_build_eq(c->dcrt, rd, nv, eq_dev, c->stream());
    return LF_OK;
}
// (a host table leaves the external-basis wrapper converted on the host; a device table changes basis in the kernel that stores it: XB with arrays)
static int build_eq_api(lf_ctx *c, const uint64_t *point, unsigned nv, uint64_t *out, Origin org) {
    if (LF_XB(c) && point && out && nv && nv <= 40) {
        XB x(c, org == Origin::device);
        int rc = build_eq_api(c, x.ext_in(point, nv), nv, out, org);
        if (rc == LF_OK && org == Origin::host) x.ext_out(out, (size_t)1 << nv);
        return rc;
    }
    if (!c || !point || !out || nv == 0 || nv > 40) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::build_eq(c->bb->p, point, nv, out, org) : ring_ops<GoldRing>::build_eq(c, point, nv, out, org);
}
int lf_build_eq(lf_ctx *c, const uint64_t *point, unsigned nv, uint64_t *out) { return build_eq_api(c, point, nv, out, Origin::host); }
int lf_build_eq_dev(lf_ctx *c, const uint64_t *point, unsigned nv, uint64_t *out) { return build_eq_api(c, point, nv, out, Origin::device); }
static int mle_eval_batch_api(lf_ctx *c, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nv, uint64_t *out, Origin org) {
    if (LF_XB(c) && tables && point && out) {
        XB x(c, true);
        int rc = mle_eval_batch_api(c, tables, ntables, len, x.ext_in(point, nv), nv, out, org);
        if (rc == LF_OK) x.ring_out(out, ntables);
        return rc;
    }
    if (!c || !tables || !point || !out || !ntables || nv == 0 || nv > 40) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::mle_eval_batch(c->bb->p, tables, ntables, len, point, nv, out, org)
                 : ring_ops<GoldRing>::mle_eval_batch(c, tables, ntables, len, point, nv, out, org);
}
int lf_mle_eval_batch(lf_ctx *c, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nv, uint64_t *out) {
    return mle_eval_batch_api(c, tables, ntables, len, point, nv, out, Origin::host);
}
int lf_mle_eval_batch_dev(lf_ctx *c, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nv, uint64_t *out) {
    return mle_eval_batch_api(c, tables, ntables, len, point, nv, out, Origin::device);
}

// ---- CCS -------------------------------------------------------------------------------------------------------------
size_t lf_lcccs_len_ring(const lf_params *p, int ring) { return lcccs_len(p, ring == LF_RING_BABYBEAR ? 9 : 3); }
size_t lf_cccs_len_ring(const lf_params *p, int) { return cccs_len(p); }
size_t lf_proof_len_ring(const lf_params *p, int ring) { return proof_len(p, ring == LF_RING_BABYBEAR ? 9 : 3); }
size_t lf_lcccs_len(const lf_params *p) { return lcccs_len(p, 3); }
size_t lf_cccs_len(const lf_params *p) { return cccs_len(p); }
size_t lf_proof_len(const lf_params *p) { return proof_len(p, 3); }

int lf_ccs_load(lf_ctx *c, const lf_params *p, const uint32_t *const *rowptr, const uint32_t *const *col, const uint64_t *const *val,
                const uint32_t *S_off, const uint32_t *S_idx, const uint64_t *cc) {
    if (LF_XB(c) && p && rowptr && col && val && S_off && S_idx && cc && p->t >= 1 && p->t <= 8 && p->s <= 30 && p->q <= 8) {
        XB x(c);
        const size_t m = (size_t)1 << p->s;
        const uint64_t *v2[8];
        for (u32 j = 0; j < p->t; j++) {
            if (!rowptr[j] || !val[j]) return LF_ERR_INVALID;
            v2[j] = x.ring_in(val[j], rowptr[j][m]);
        }
        return lf_ccs_load(c, p, rowptr, col, v2, S_off, S_idx, x.ring_in(cc, p->q));
    }
    if (!c || !p || !rowptr || !col || !val || !S_off || !S_idx || !cc) return LF_ERR_INVALID;
    if (c->bb) { RET(lfbb::ccs_envelope(p)); return ring_ops<BbRing>::ccs_load(c->bb->p, p, rowptr, col, val, S_off, S_idx, cc); }
    if (p->s < 3 || p->s > LF_S_MAX || p->t == 0 || p->t > 8 || p->q == 0 || p->q > 8 || p->K == 0 || p->K > 32 || p->L == 0 || p->L > 8 ||
        p->d > 7 || p->wit_len == 0)
        return LF_ERR_UNSUPPORTED;
    // b = 2: the bit-plane kernels of the reference Goldilocks rows; b = 4, 8, 16: the small-base path (lf_sb.h), one unsharded GPU
    if (p->b != 2 && !sb_base_ok(p->b)) return LF_ERR_UNSUPPORTED;
    if (p->b != 2 && (c->sh_world > 1 || c->comm[0].model || p->K > 11)) return LF_ERR_UNSUPPORTED;   // (K - 1 <= 10 planes of one commit launch)
    // B = 2^32 (config.toml:158): balanced digits lie in [-2^31, 2^31]; the int32 planes hold all of them but +2^31 exactly, which the ingest
    // rejects (LF_ERR_UNSUPPORTED) -- one value in 2^32 per digit
    if (!pow2(p->B) || p->B > (1ULL << 32)) return LF_ERR_UNSUPPORTED;
    // K base-b digits must cover |coeff| <= B/2 under the active digit rule (checked again where a step starts: the rule may change after the load)
    if (!sb_digits_cover(p->b, p->K, p->B, c->digit_mode)) return LF_ERR_UNSUPPORTED;
    return ring_ops<GoldRing>::ccs_load(c, p, rowptr, col, val, S_off, S_idx, cc);
}
int lf_spmv(lf_ctx *c, unsigned j, const uint64_t *z, uint64_t *out) {
    XbArrays xa(c);
    if (!c || !z || !out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::spmv(c->bb->p, j, z, out) : ring_ops<GoldRing>::spmv(c, j, z, out);
}
int lf_spmv_dev(lf_ctx *c, unsigned j, const uint64_t *z, uint64_t *out) {
    if (!c || !z || !out) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::spmv(c->bb->p, j, z, out, Origin::device) : ring_ops<GoldRing>::spmv(c, j, z, out, Origin::device);
}

// ---- witnesses ---------------------------------------------------------------------------------------------------------
// ---- ingestion next to a running fold step (a chain's next witness: upload over PCIe, ICRT and gadget decomposition on the lowest-priority stream while the
// step before it folds).  Goldilocks contexts in the default basis run it on lane 2 (own stream, own buffers, c->io_mu instead of c->mu: the constraint system
// must not be reloaded meanwhile); every other configuration runs the blocking call on the worker thread -- the same witness, no overlap promised.
struct lf_witness_job {
    std::future<int> fut;
    lf_witness *w = nullptr;
};
int lf_witness_from_w_ccs_begin(lf_ctx *c, const uint64_t *w_ccs, lf_witness_job **job) {
    if (!c || !w_ccs || !job) return LF_ERR_INVALID;
    if (!c->have_ccs_any()) return LF_ERR_STATE;
    lf_witness_job *j = new lf_witness_job();
    c->io_jobs.fetch_add(1);
    j->fut = std::async(std::launch::async, [c, w_ccs, j]() -> int {
        struct Done { lf_ctx *c; ~Done() { c->io_jobs.fetch_sub(1); } } done{c};
        if (c->bb || c->xb.on) return lf_witness_from_w_ccs(c, w_ccs, &j->w);
        std::lock_guard<std::mutex> g(c->io_mu);
        if (hipSetDevice(c->device) != hipSuccess) return LF_ERR_HIP;
        t_lane = 2;
        return ring_ops<GoldRing>::witness_from_w_ccs_lane(c, w_ccs, &j->w);
    });
    *job = j;
    return LF_OK;
}
int lf_witness_job_finish(lf_witness_job *job, lf_witness **out) {
    if (!job) return LF_ERR_INVALID;
    const int rc = job->fut.valid() ? job->fut.get() : LF_ERR_STATE;
    if (rc == LF_OK && out) *out = job->w;
    else if (job->w) lf_witness_free(job->w);      // (a caller that abandons the job passes out = NULL)
    delete job;
    return rc;
}
int lf_witness_from_w_ccs(lf_ctx *c, const uint64_t *w_ccs, lf_witness **out) {
    XbArrays xa(c);
    if (!c || !w_ccs || !out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_from_w_ccs(c->bb->p, w_ccs, out) : ring_ops<GoldRing>::witness_from_w_ccs(c, w_ccs, out);
}
int lf_witness_from_f_coeff(lf_ctx *c, const uint64_t *f_coeff, lf_witness **out) {
    if (!c || !f_coeff || !out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_from_f_coeff(c->bb->p, f_coeff, out) : ring_ops<GoldRing>::witness_from_f_coeff(c, f_coeff, out);
}
int lf_witness_from_f(lf_ctx *c, const uint64_t *f_ntt, lf_witness **out) {
    XbArrays xa(c);
    if (!c || !f_ntt || !out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_from_f(c->bb->p, f_ntt, out) : ring_ops<GoldRing>::witness_from_f(c, f_ntt, out);
}
int lf_witness_get_f_coeff(lf_ctx *c, const lf_witness *w, uint64_t *out) {
    if (!c || !w || !out || w->ctx != c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_get_f_coeff(c->bb->p, w, out) : ring_ops<GoldRing>::witness_get_f_coeff(c, w, out);
}
int lf_witness_get_f(lf_ctx *c, const lf_witness *w, uint64_t *out) {
    XbArrays xa(c);
    if (!c || !w || !out || w->ctx != c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_get_f(c->bb->p, w, out) : ring_ops<GoldRing>::witness_get_f(c, w, out);
}
int lf_witness_get_w_ccs(lf_ctx *c, const lf_witness *w, uint64_t *out) {
    XbArrays xa(c);
    if (!c || !w || !out || w->ctx != c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_get_w_ccs(c->bb->p, w, out) : ring_ops<GoldRing>::witness_get_w_ccs(c, w, out);
}
int lf_witness_from_w_ccs_dev(lf_ctx *c, const uint64_t *w_ccs, lf_witness **out) {
    if (!c || !w_ccs || !out) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::witness_from_w_ccs(c->bb->p, w_ccs, out, Origin::device) : ring_ops<GoldRing>::witness_from_w_ccs(c, w_ccs, out, Origin::device);
}
int lf_witness_from_f_coeff_dev(lf_ctx *c, const uint64_t *f_coeff, lf_witness **out) {
    if (!c || !f_coeff || !out) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::witness_from_f_coeff(c->bb->p, f_coeff, out, Origin::device) : ring_ops<GoldRing>::witness_from_f_coeff(c, f_coeff, out, Origin::device);
}
int lf_witness_from_f_dev(lf_ctx *c, const uint64_t *f_ntt, lf_witness **out) {
    if (!c || !f_ntt || !out) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::witness_from_f(c->bb->p, f_ntt, out, Origin::device) : ring_ops<GoldRing>::witness_from_f(c, f_ntt, out, Origin::device);
}
int lf_witness_get_f_coeff_dev(lf_ctx *c, const lf_witness *w, uint64_t *out) {
    if (!c || !w || !out || w->ctx != c) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::witness_get_f_coeff(c->bb->p, w, out, Origin::device) : ring_ops<GoldRing>::witness_get_f_coeff(c, w, out, Origin::device);
}
int lf_witness_get_f_dev(lf_ctx *c, const lf_witness *w, uint64_t *out) {
    if (!c || !w || !out || w->ctx != c) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::witness_get_f(c->bb->p, w, out, Origin::device) : ring_ops<GoldRing>::witness_get_f(c, w, out, Origin::device);
}
int lf_witness_get_w_ccs_dev(lf_ctx *c, const lf_witness *w, uint64_t *out) {
    if (!c || !w || !out || w->ctx != c) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::witness_get_w_ccs(c->bb->p, w, out, Origin::device) : ring_ops<GoldRing>::witness_get_w_ccs(c, w, out, Origin::device);
}
int lf_witness_commit(lf_ctx *c, const lf_witness *w, uint64_t *cm_out) {
    if (LF_XB(c) && w && cm_out) { XB x(c); int rc = lf_witness_commit(c, w, cm_out); if (rc == LF_OK) x.ring_out(cm_out, c->core_any().kappa); return rc; }
    if (!c || !w || !cm_out || w->ctx != c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_commit(c->bb->p, w, cm_out) : ring_ops<GoldRing>::witness_commit(c, w, cm_out);
}
// ---- decomposed witnesses: the wit_s of LFDecompositionProver::prove and the w_s of LFFoldingProver::prove as handles (lf_ring_host.h: witness_decompose /
// witness_recompose; one body for both rings).  The two provers with parts are the calls above and below composed: every refusal of the parts comes before the
// prover sees its transcript.
// every output handle is NULL after an error: cleared before the first check that can refuse (a context without a CCS has no K: nothing to clear)
static void parts_clear(lf_ctx *c, lf_witness **parts_out) {
    if (c && parts_out && c->have_ccs_any())
        for (u32 k = 0, K = c->params_any().K; k < K; k++) parts_out[k] = nullptr;
}
int lf_witness_decompose(lf_ctx *c, const lf_witness *wit, lf_witness **parts_out) {
    parts_clear(c, parts_out);
    if (!c || !wit || !parts_out || wit->ctx != c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_decompose(c->bb->p, wit, parts_out) : ring_ops<GoldRing>::witness_decompose(c, wit, parts_out);
}
int lf_witness_recompose(lf_ctx *c, const lf_witness *const *parts, unsigned count, lf_witness **out) {
    if (out) *out = nullptr;
    if (!c || !parts || !out) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_recompose(c->bb->p, parts, count, out) : ring_ops<GoldRing>::witness_recompose(c, parts, count, out);
}
int lf_decomposition_prove_parts(lf_ctx *c, lf_transcript *t, const uint64_t *lcccs, const lf_witness *wit, uint64_t *lcccs_s_out, uint64_t *dec_proof_out,
                                 lf_witness **parts_out) {
    parts_clear(c, parts_out);
    if (!c || !t || !lcccs || !wit || !dec_proof_out || !parts_out || wit->ctx != c || (c->bb != nullptr) != (t->bb != nullptr)) return LF_ERR_INVALID;
    RET(lf_witness_decompose(c, wit, parts_out));   // the parts first: whatever refuses them refuses the call before the first absorb
    const int rc = lf_decomposition_prove(c, t, lcccs, wit, lcccs_s_out, dec_proof_out);
    if (rc != LF_OK)
        for (u32 k = 0, K = c->params_any().K; k < K; k++) { lf_witness_free(parts_out[k]); parts_out[k] = nullptr; }
    return rc;
}
int lf_folding_prove_parts(lf_ctx *c, lf_transcript *t, const uint64_t *lcccs_s, const lf_witness *const *w_s, unsigned count, uint64_t *lcccs_out,
                           lf_witness **w_out, uint64_t *fold_proof_out) {
    if (w_out) *w_out = nullptr;
    if (!c || !t || !lcccs_s || !w_s || !lcccs_out || !w_out || !fold_proof_out || (c->bb != nullptr) != (t->bb != nullptr)) return LF_ERR_INVALID;
    if (!c->have_ccs_any()) return LF_ERR_STATE;
    const u32 K = c->params_any().K;
    if (count != 2 * K) return LF_ERR_INVALID;
    lf_witness *side[2] = {nullptr, nullptr};   // the two sums: the accumulator's, then the fresh instance's
    int rc = lf_witness_recompose(c, w_s, K, &side[0]);
    if (rc == LF_OK) rc = lf_witness_recompose(c, w_s + K, K, &side[1]);
    if (rc == LF_OK) rc = lf_folding_prove(c, t, lcccs_s, side[0], side[1], lcccs_out, w_out, fold_proof_out);
    lf_witness_free(side[0]);
    lf_witness_free(side[1]);
    if (rc != LF_OK && *w_out) { lf_witness_free(*w_out); *w_out = nullptr; }
    return rc;
}
// ---- witness tables (lfhip_tables.h; lf_ring_host.h: one body per call for both spellings and both rings).  In an external basis the arrays change basis in
// the relayout kernels (f-hat needs none: a constant slot is c e_0 in any basis), x and the points on the host
static int witness_get_fhat_api(lf_ctx *c, const lf_witness *const *wits, unsigned count, uint64_t *out, Origin org) {
    if (!c || !wits || !out) return LF_ERR_INVALID;
    for (unsigned w = 0; w < count; w++)
        if (!wits[w] || wits[w]->ctx != c) return LF_ERR_INVALID;
    return c->bb ? ring_ops<BbRing>::witness_get_fhat(c->bb->p, wits, count, out, org) : ring_ops<GoldRing>::witness_get_fhat(c, wits, count, out, org);
}
int lf_witness_get_fhat(lf_ctx *c, const lf_witness *const *wits, unsigned count, uint64_t *out) { return witness_get_fhat_api(c, wits, count, out, Origin::host); }
int lf_witness_get_fhat_device(lf_ctx *c, const lf_witness *const *wits, unsigned count, uint64_t *out) {
    return witness_get_fhat_api(c, wits, count, out, Origin::device);
}
// z and M z: x is small -- validated, then converted by the wrapper
static int witness_z_api(lf_ctx *c, const lf_witness *w, const uint64_t *x, uint64_t *out, bool mz, Origin org) {
    if (!c || !w || !x || !out || w->ctx != c) return LF_ERR_INVALID;
    if (LF_XB(c) && c->have_ccs_any()) {   // (x is read only once the handle is known to belong to the loaded system: it holds l elements of THAT system)
        if (w->N != c->N_any()) return LF_ERR_INVALID;
        const size_t l = c->params_any().l, words = l * (size_t)lf_ring_words(lf_ctx_ring(c));
        for (size_t i = 0; i < words; i++)
            if (x[i] >= lf_ring_modulus(lf_ctx_ring(c))) return LF_ERR_INVALID;
        XB xb(c, true);
        return witness_z_api(c, w, xb.ring_in(x, l), out, mz, org);
    }
    if (mz) return c->bb ? ring_ops<BbRing>::witness_mz(c->bb->p, w, x, out, org) : ring_ops<GoldRing>::witness_mz(c, w, x, out, org);
    return c->bb ? ring_ops<BbRing>::witness_get_z(c->bb->p, w, x, out, org) : ring_ops<GoldRing>::witness_get_z(c, w, x, out, org);
}
int lf_witness_get_z(lf_ctx *c, const lf_witness *w, const uint64_t *x, uint64_t *out) { return witness_z_api(c, w, x, out, false, Origin::host); }
int lf_witness_get_z_device(lf_ctx *c, const lf_witness *w, const uint64_t *x, uint64_t *out) { return witness_z_api(c, w, x, out, false, Origin::device); }
int lf_witness_mz(lf_ctx *c, const lf_witness *w, const uint64_t *x, uint64_t *out) { return witness_z_api(c, w, x, out, true, Origin::host); }
int lf_witness_mz_device(lf_ctx *c, const lf_witness *w, const uint64_t *x, uint64_t *out) { return witness_z_api(c, w, x, out, true, Origin::device); }
static int spmv_t_api(lf_ctx *c, unsigned j, const uint64_t *v, uint64_t *out, Origin org) {
    if (!c || !v || !out) return LF_ERR_INVALID;
    XbArrays xa(c);
    return c->bb ? ring_ops<BbRing>::spmv_t(c->bb->p, j, v, out, org) : ring_ops<GoldRing>::spmv_t(c, j, v, out, org);
}
int lf_spmv_t(lf_ctx *c, unsigned j, const uint64_t *v, uint64_t *out) { return spmv_t_api(c, j, v, out, Origin::host); }
int lf_spmv_t_device(lf_ctx *c, unsigned j, const uint64_t *v, uint64_t *out) { return spmv_t_api(c, j, v, out, Origin::device); }
static int mle_fix_variables_api(lf_ctx *c, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nfix, uint64_t *out, Origin org) {
    if (!c || !tables || !point || !out) return LF_ERR_INVALID;
    if (LF_XB(c)) {   // (the shape first: the point holds nfix challenges only if nfix is one the body accepts)
        if (len < 2 || (len & (len - 1)) || !nfix || nfix >= 64 || ((size_t)1 << nfix) > len) return LF_ERR_INVALID;
        for (size_t i = 0, words = (size_t)nfix * lf_ring_tau(lf_ctx_ring(c)); i < words; i++)
            if (point[i] >= lf_ring_modulus(lf_ctx_ring(c))) return LF_ERR_INVALID;
        XB xb(c, true);
        return mle_fix_variables_api(c, tables, ntables, len, xb.ext_in(point, nfix), nfix, out, org);
    }
    return c->bb ? ring_ops<BbRing>::mle_fix_variables(c->bb->p, tables, ntables, len, point, nfix, out, org)
                 : ring_ops<GoldRing>::mle_fix_variables(c, tables, ntables, len, point, nfix, out, org);
}
int lf_mle_fix_variables(lf_ctx *c, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nfix, uint64_t *out) {
    return mle_fix_variables_api(c, tables, ntables, len, point, nfix, out, Origin::host);
}
int lf_mle_fix_variables_device(lf_ctx *c, const uint64_t *tables, size_t ntables, size_t len, const uint64_t *point, unsigned nfix, uint64_t *out) {
    return mle_fix_variables_api(c, tables, ntables, len, point, nfix, out, Origin::device);
}
// (not part of the ABI: tests and measurements) the heavy-column threshold of lf_spmv_t the NEXT lf_ccs_load builds its work lists with (0: the shipped one);
// returns the one in force for the loaded system
extern "C" unsigned lfdbg_spmv_t_heavy_min(lf_ctx *c, unsigned next) {
    if (!c) return 0;
    CtxCoreBase &k = c->core_any();
    std::lock_guard<std::mutex> g(k.mu);
    k.spmvt_min_next = next ? next : lfk::SPMV_T_HEAVY;
    return k.spmvt_min;
}
// pool of recycled witness-plane buffers: process-wide (a witness may be freed after its context), keyed by device and size
namespace {
struct PoolEnt { int device; size_t bytes; int32_t *p; };
std::mutex g_pool_mu;
std::vector<PoolEnt> g_pool;
}  // namespace
int lf_planes_alloc(lf_ctx *c, size_t bytes, int32_t **out) {
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); i++)
            if (g_pool[i].device == c->device && g_pool[i].bytes == bytes) {
                *out = g_pool[i].p;
                g_pool.erase(g_pool.begin() + (long)i);
                return LF_OK;
            }
    }
    return lf_dev_malloc(out, bytes) == hipSuccess ? LF_OK : LF_ERR_HIP;
}
static void planes_release_dev(int device, size_t bytes, int32_t *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        if (g_pool.size() < 9) { g_pool.push_back({device, bytes, p}); return; }   // planes, f and w_ccs of up to three witnesses
    }
    (void)hipFree(p);
}
void lf_planes_release(lf_ctx *c, size_t bytes, int32_t *p) { planes_release_dev(c->device, bytes, p); }
static void planes_pool_drop(int device) {
    std::lock_guard<std::mutex> g(g_pool_mu);
    for (size_t i = 0; i < g_pool.size();)
        if (g_pool[i].device == device) { (void)hipFree(g_pool[i].p); g_pool.erase(g_pool.begin() + (long)i); }
        else i++;
}
void lf_witness_free(lf_witness *w) {
    if (!w) return;
    // the context may be gone already (callers close contexts before their witnesses): use only what the handle itself carries
    (void)hipSetDevice(w->device);
    planes_release_dev(w->device, w->plane_bytes, w->planes);
    planes_release_dev(w->device, w->f_bytes, (int32_t *)w->f_ntt);
    planes_release_dev(w->device, w->w_bytes, (int32_t *)w->w_ccs);
    delete w;
}

// ---- transcript ------------------------------------------------------------------------------------------------------------
lf_transcript *lf_transcript_new(void) { return new lf_transcript(); }
lf_transcript *lf_transcript_new_ring(int ring) {
    if (ring == LF_RING_GOLDILOCKS) return new lf_transcript();
    if (ring != LF_RING_BABYBEAR) return nullptr;
    lf_transcript *t = new lf_transcript();
    t->bb = new lfbb::BbTranscript();
    return t;
}
lf_transcript *lf_transcript_clone(const lf_transcript *t) { return t ? new lf_transcript(*t) : nullptr; }
void lf_transcript_free(lf_transcript *t) { delete t; }
void lf_transcript_absorb_fq(lf_transcript *t, const uint64_t *x, size_t n) {
    if (t->bb) t->bb->absorb_fq(x, n);
    else t->t.absorb_fq(x, n);
}
void lf_transcript_absorb_ring(lf_transcript *t, const uint64_t *e, size_t n) {
    if (t->bb) t->bb->absorb_ring(e, n);
    else t->t.absorb_ring(e, n);
}
void lf_transcript_get_challenge(lf_transcript *t, uint64_t *o) {
    if (t->bb) {
        lfbb::H9 c = t->bb->get_challenge();
        memcpy(o, c.c, sizeof(c.c));
        return;
    }
    Fq3 c = t->t.get_challenge();
    o[0] = c.c[0]; o[1] = c.c[1]; o[2] = c.c[2];
}
void lf_transcript_get_short_challenge(lf_transcript *t, uint64_t *o) {
    if (t->bb) t->bb->get_short_challenge(o);
    else t->t.get_short_challenge(o);
}
void lf_transcript_squeeze_bytes(lf_transcript *t, uint8_t *out, size_t n) {
    // CryptographicSponge::squeeze_bytes of the arkworks-0.4 PoseidonSponge (Transcript::squeeze_bytes, transcript/poseidon.rs:62-64): ceil(n / usable) field
    // elements, usable = (modulus bits - 1) / 8 low little-endian bytes of each (7 Goldilocks, 3 BabyBear), truncated to n
    if (!t || !out || !n) return;
    const size_t usable = t->bb ? 3 : 7, ne = (n + usable - 1) / usable;
    std::vector<u64> e(ne);
    if (t->bb) t->bb->squeeze(e.data(), ne);
    else t->t.squeeze(e.data(), ne);
    for (size_t i = 0, o = 0; i < ne && o < n; i++)
        for (size_t j = 0; j < usable && o < n; j++) out[o++] = (uint8_t)(e[i] >> (8 * j));
}
void lf_poseidon_permute(uint64_t *state, int plain) {
    if (plain == 2) Transcript::permute_scalar(state);
    else if (plain) Transcript::permute_plain(state);
    else Transcript::permute(state);
}
void lf_poseidon_permute_ring(uint64_t *state, int plain, int ring) {
    if (ring == LF_RING_BABYBEAR) {
        if (plain == 2) lfbb::BbTranscript::permute_scalar(state);
        else if (plain) lfbb::BbTranscript::permute_plain(state);
        else lfbb::BbTranscript::permute(state);
    } else lf_poseidon_permute(state, plain);
}
void lf_poseidon_params(uint64_t *ark, uint64_t *mds) {
    const u64 *a, *m;
    Transcript::params(&a, &m);
    memcpy(ark, a, 720 * 8);
    memcpy(mds, m, 576 * 8);
}
void lf_poseidon_params_ring(uint64_t *ark, uint64_t *mds, int ring) {
    const u64 *a, *m;
    if (ring == LF_RING_BABYBEAR) lfbb::BbTranscript::params(&a, &m);
    else Transcript::params(&a, &m);
    memcpy(ark, a, 720 * 8);
    memcpy(mds, m, 576 * 8);
}

int lf_last_phase_ms(lf_ctx *c, float *out) {
    if (!c || !out) return LF_ERR_INVALID;
    for (int i = 0; i < LF_N_PHASES; i++) out[i] = c->core_any().phase_ms[i];
    return LF_OK;
}
// wall-clock marks of the caller thread during the last lf_fold_step (Goldilocks driver): name i (NUL-terminated, at most 31 characters) at
// names + 32 i, ms[i] = milliseconds since the start of the step.  Returns the number of marks written (<= max_marks), < 0 on error.
int lf_last_timeline(lf_ctx *c, char *names, double *ms, int max_marks) {
    if (!c || !names || !ms || max_marks < 0) return LF_ERR_INVALID;
    if (c->bb) return 0;
    int n = 0;
    for (auto &m : c->tl_marks) {
        if (n >= max_marks) break;
        const char *w = m.first;
        while (*w == ' ') w++;
        snprintf(names + 32 * n, 32, "%s", w);
        ms[n++] = m.second;
    }
    return n;
}
// measurement hook of tools/gpu_i8prof.sh (not part of the prover interface, not declared in lfhip.h): per-phase clock totals of the last commit
// launch made with LF_I8_PROF set
int lf_abi_version(void) { return LFHIP_ABI_VERSION; }
int lf_debug_i8_prof(uint64_t *out64) {   // (LF_I8G_PROF set: the table of the general-commit kernel instead)
    if (!out64) return LF_ERR_INVALID;
    return getenv("LF_I8G_PROF") ? ajtai_i8g_read_prof((unsigned long long *)out64) : ajtai_i8_read_prof((unsigned long long *)out64);
}
// (not part of the ABI: tools/i8g_prof.py) per-workgroup loop durations of the last profiled general commit
extern "C" int lfdbg_i8g_wg(unsigned int *out512) { return out512 ? ajtai_i8g_read_wg(out512) : -1; }
// (not part of the ABI: tests) digit planes the gadget commitments use for a power-of-two base (ring: LF_RING_*)
extern "C" unsigned lfdbg_i8g_planes_base(int ring, uint64_t base) { return ajtai_i8g_planes_base(ring == LF_RING_BABYBEAR ? ajtai_i8_babybear() : ajtai_i8_goldilocks(), base); }
// (not part of the ABI: tests) the trailing-empty-row schedule of lf_live_rows.h: live_rows of the loaded CCS (-1: none / BabyBear), of host row pointers, and the
// live entries of the linearization tables of rounds 1 .. rounds for m rows (low != 0: the LF_LIVE_ROWS_LOW threshold and granule); the rounds of the last
// linearization that ran on a live prefix
extern "C" long long lfdbg_live_rows(lf_ctx *c) { return c && !c->bb && c->have_ccs ? (long long)c->live_rows : -1; }
extern "C" size_t lfdbg_live_rows_csr(unsigned t, size_t m, const uint32_t *const *rowptr) { return lflive::live_rows(t, m, rowptr); }
extern "C" void lfdbg_live_schedule(size_t m, size_t live, int low, unsigned rounds, size_t *out) {
    const lflive::Plan p = low ? lflive::plan(m, live, lflive::GRANULE_LOW, lflive::MIN_M_LOW) : lflive::plan(m, live, lflive::GRANULE, lflive::MIN_M);
    for (unsigned i = 1; i <= rounds; i++) out[i - 1] = lflive::entries(p, i);
}
extern "C" int lfdbg_last_lin_live_rounds(lf_ctx *c) { return c && !c->bb ? (int)c->lin_live_rounds : -1; }
int lf_last_fold_paths(lf_ctx *c, unsigned *sv_round_mask) {
    if (!c || !sv_round_mask) return LF_ERR_INVALID;
    *sv_round_mask = c->core_any().sv_round_mask;
    return LF_OK;
}
int lf_last_fold_split_rounds(lf_ctx *c, unsigned *round_mask) {
    if (!c || !round_mask) return LF_ERR_INVALID;
    *round_mask = c->core_any().fold_split_mask;
    return LF_OK;
}
int lf_last_lin_split_rounds(lf_ctx *c, unsigned *rounds) {
    if (!c || !rounds) return LF_ERR_INVALID;
    *rounds = c->bb ? 0u : c->lin_split_rounds;
    return LF_OK;
}
int lf_last_kernel_stats(lf_ctx *c, float *fold_ms, int *fold_n, float *aj_ms, int *aj_n) {
    if (!c) return LF_ERR_INVALID;
    const CtxCoreBase &k = c->core_any();
    if (fold_ms) *fold_ms = k.k_fold_ms;
    if (fold_n) *fold_n = k.k_fold_n;
    if (aj_ms) *aj_ms = k.k_ajtai_ms;
    if (aj_n) *aj_n = k.k_ajtai_n;
    return LF_OK;
}

// ---- host-side verifier ---------------------------------------------------------------------------------------
// the host ring with the default tables: what the context-free verifiers compute in
static const HostRing &default_host_ring() {
    static const HostRing *hr = [] {
        HostRing *g = new HostRing();
        u64 nr, y[24];
        default_ring(&nr, y);
        build_crt_tables(nr, y, g->T);
        return g;
    }();
    return *hr;
}
int lf_verify_host(int ring, const lf_params *p, const uint32_t *S_off, const uint32_t *S_idx, const uint64_t *c, lf_transcript *t,
                   const uint64_t *acc, const uint64_t *cm_i, const uint64_t *proof, uint64_t *lcccs_out, int *failed_stage) {
    if (!p || !S_off || !S_idx || !c || !t || !acc || !cm_i || !proof || !lcccs_out) return LF_ERR_INVALID;
    if (p->s == 0 || p->s > 40 || p->K == 0 || p->K > 32 || p->q == 0 || p->q > 8 || p->t == 0 || p->t > 16) return LF_ERR_UNSUPPORTED;
    if (((size_t)1 << p->s) < (size_t)p->wit_len * p->L) return LF_ERR_SIZE_BOUNDS;   // sanity_check, nifs.rs:165-173
    if (failed_stage) *failed_stage = 0;
    if (ring == LF_RING_BABYBEAR) return t->bb ? lfbb::bb_verify_host(p, S_off, S_idx, c, *t->bb, acc, cm_i, proof, lcccs_out, failed_stage) : LF_ERR_INVALID;
    if (ring != LF_RING_GOLDILOCKS || t->bb) return LF_ERR_INVALID;
    const GoldV gv{default_host_ring()};
    lfv::Verifier<GoldV> V(gv, *p, S_off, S_idx, c);
    int rc = V.verify(t->t, acc, cm_i, proof, lcccs_out);
    if (failed_stage) *failed_stage = V.stage;
    return rc;
}

// MLSumcheck::verify_as_subprotocol (utils/sumcheck.rs:84-104) on the host: lfv::sumcheck_verify, the body the NIFS verifier runs its two sumchecks through
int lf_mlsumcheck_verify(int ring, lf_transcript *t, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum, const uint64_t *msgs, uint64_t *point_out,
                         uint64_t *expected_out) {
    if (!t || !claimed_sum || !msgs || !point_out || !expected_out) return LF_ERR_INVALID;
    if (ring != LF_RING_GOLDILOCKS && ring != LF_RING_BABYBEAR) return LF_ERR_INVALID;
    if ((ring == LF_RING_BABYBEAR) != (t->bb != nullptr)) return LF_ERR_INVALID;
    if (nvars < 1 || nvars > lfml::MAX_NVARS || degree < 1 || degree > lfml::MAX_DEGREE) return LF_ERR_UNSUPPORTED;
    if (ring == LF_RING_BABYBEAR) return lfbb::bb_mlsumcheck_verify(*t->bb, nvars, degree, claimed_sum, msgs, point_out, expected_out);
    return lfv::mlsumcheck_verify(GoldV{default_host_ring()}, t->t, nvars, degree, claimed_sum, msgs, point_out, expected_out);
}
