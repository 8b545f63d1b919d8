// lf_ctx_core.h -- what a context is on BOTH rings, defined once: the two prover lanes' streams, the named device-buffer cache, the pinned download buffers,
// the event pool behind the timing read-outs, the resident matrix and constraint system, the sharding rank, the sumcheck-ABI state and the masks the read-outs
// report.  lf_ctx (Goldilocks, lf_ctx.h) and lfbb::BbCtxImpl (BabyBear, bb_ctx.h) derive from CtxCore<device word> and keep only what is really theirs.
// Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lfhip.h"
#include "lf_common.h"
#include "lf_mlsumcheck.h"
#include "lf_spmv_t_plan.h"

struct lf_witness;

// lanes of a context: 0 = the caller's thread, 1 = the helper lane of a fold step (left decomposition), 2 = witness ingestion next to a running step
// (Goldilocks only).  Every lane-indexed array has a slot for each of them.
constexpr int LF_NLANES = 3;

struct EvPair { hipEvent_t a, b; };

struct CtxCoreBase {
    int device = 0;
    hipStream_t st_lane[LF_NLANES] = {nullptr, nullptr, nullptr};   // [2]: the ingestion stream, null on a ring without lane 2
    std::mutex mu, buf_mu, ev_mu;
    int digit_mode = 0;   // balanced-digit rule of base-B decompositions (lf_set_digit_mode)
    Tunables tn;          // environment switches, re-read at the start of every linearize / fold step / general commit
    uint32_t lin_blocks = 0;   // grid bound of the linearization rounds while a fold step's commit chain runs on the other lane (0 = none)
    // Ajtai matrix: coefficient form, bytes in int8-MFMA operand order (lf_ajtai_i8.hip), row chunks of i8_kc rows.  nA = columns held by this rank, starting at
    // global column A_col0 of nA_total.  All of it is published together, by a successful install only (ring_ops::ajtai_install)
    bool A_loaded = false;
    unsigned char *dAb = nullptr;
    uint32_t i8_nch = 0, i8_kc = 0;
    uint32_t kappa = 0;
    size_t nA = 0, nA_total = 0, A_col0 = 0;
    int sh_rank = 0, sh_world = 1;   // intra-step sharding: mirror the communicator's rank / world
    // CCS
    bool have_ccs = false;
    lf_params P{};
    size_t N = 0, m = 0, n = 0;
    std::vector<uint32_t *> d_rowptr, d_col, d_colptr, d_rowidx;
    // lf_spmv_t: per matrix, the work list of its heavy columns on the device (lf_spmv_t_plan.h; null without heavy columns) and its two lengths; the threshold
    // the lists of the loaded system were built with, and the one the next lf_ccs_load takes (a test hook moves it: lfdbg_spmv_t_heavy_min)
    std::vector<uint32_t *> d_spmvt_plan;
    std::vector<uint32_t> spmvt_items, spmvt_cols;
    uint32_t spmvt_min = lfk::SPMV_T_HEAVY, spmvt_min_next = lfk::SPMV_T_HEAVY;
    uint64_t setup_gen = 0;   // counts the times the matrix or the constraint system was dropped (a reload drops first): how an lf_prover sees a reload of equal shape
    // sumcheck ABI state: linearization (lf_sumcheck_lin_*) and folding (lf_sumcheck_fold_*)
    int sc_round = -1, sc_cur = 0;
    size_t sc_n = 0;
    int sf_round = -1, sf_cur = 0;
    size_t sf_n = 0;
    // the generic sumcheck (lf_mlsumcheck_*), a state of its own with buffers of its own (ml_*): rounds done (-1: none active), the buffer the current tables
    // are in, their length, and the copied descriptor as the round kernel takes it
    int ml_round = -1, ml_cur = 0;
    size_t ml_n = 0;
    uint32_t ml_nvars = 0, ml_T = 0;
    lfml::Desc ml_desc{};
    // v_s of the linearized instance computed inside the linearization (v = sum_k 2^k v_s[k]); reused by the right decomposition of the same fold step
    const lf_witness *vs_wit = nullptr;
    bool vs_keep = false;            // set by the fold step around its linearization: only there the decomposition that follows uses the same point
    uint64_t *vs_dev = nullptr;
    // Second-stream hand-off of the fold step (the helper lane's idle stream next to the caller's): fork(from, to) lets `to` continue behind what `from` has queued,
    // guarded by ev_prep[0]; join(from, to) is the way back, guarded by ev_prep[1] (join_mark + join_wait where the wait comes later or inside a launcher).
    // One stream on both ends: nothing to do.  The events are created once.
    hipEvent_t ev_prep[2] = {nullptr, nullptr};
    hipEvent_t prep_mark(int e, hipStream_t from) {   // nullptr: HIP error
        for (int i = 0; i < 2; i++)
            if (!ev_prep[i] && hipEventCreateWithFlags(&ev_prep[i], hipEventDisableTiming) != hipSuccess) return nullptr;
        return hipEventRecord(ev_prep[e], from) == hipSuccess ? ev_prep[e] : nullptr;
    }
    int prep_wait(int e, hipStream_t to) { return hipStreamWaitEvent(to, ev_prep[e], 0) == hipSuccess ? LF_OK : LF_ERR_HIP; }
    int fork(hipStream_t from, hipStream_t to) { return from == to ? LF_OK : (prep_mark(0, from) ? prep_wait(0, to) : LF_ERR_HIP); }
    int join(hipStream_t from, hipStream_t to) { return from == to ? LF_OK : (prep_mark(1, from) ? prep_wait(1, to) : LF_ERR_HIP); }
    hipEvent_t join_mark(hipStream_t from) { return prep_mark(1, from); }
    int join_wait(hipStream_t to) { return prep_wait(1, to); }
    unsigned sv_round_mask = 0;      // rounds of the last folding sumcheck that ran as int8 GEMMs (bit i-1 = round i; lf_last_fold_paths)
    unsigned fold_split_mask = 0;    // table rounds of the last folding sumcheck that ran in the split eq form (lf_last_fold_split_rounds)
    // measurement
    float phase_ms[LF_N_PHASES] = {0};
    float k_fold_ms = 0, k_ajtai_ms = 0;
    int k_fold_n = 0, k_ajtai_n = 0;
    double host_tr_ms = 0;

    virtual int lane() const = 0;    // the one hook: lf_ctx answers with the calling thread's t_lane, BbCtxImpl with the lane its driver set
    hipStream_t stream() const { return st_lane[lane()]; }

    // ---- named device buffers, one set per lane -------------------------------------------------------------------------------------------------------
    std::map<std::string, DevBuf> bufs;
    std::string lane_name(const std::string &name) const {
        const int l = lane();
        return l ? (l == 1 ? "lane1:" : "lane2:") + name : name;
    }
    int buf(const std::string &name, size_t bytes, void **out) {
        DevBuf *b;
        {
            std::lock_guard<std::mutex> g(buf_mu);
            b = &bufs[lane_name(name)];  // std::map nodes are stable
        }
        int rc = b->ensure(bytes);
        *out = b->p;
        return rc;
    }
    // give a set-up scratch buffer back (caller has synchronised the stream that used it)
    void drop_buf(const std::string &name) {
        std::lock_guard<std::mutex> g(buf_mu);
        auto it = bufs.find(lane_name(name));
        if (it != bufs.end()) { it->second.release(); bufs.erase(it); }
    }
    template <class T>
    int tbuf(const std::string &name, size_t count, T **out) {
        void *p;
        int rc = buf(name, count * sizeof(T), &p);
        *out = (T *)p;
        return rc;
    }
    // ---- pinned host memory per lane: downloads (pin) and the message of a sumcheck round (round_out: device-mapped, the round kernels write it directly) ----
    uint64_t *h_pin_lane[LF_NLANES] = {nullptr, nullptr, nullptr};
    size_t h_pin_words_lane[LF_NLANES] = {0, 0, 0};
    uint64_t *h_round[LF_NLANES] = {nullptr, nullptr, nullptr};
    uint64_t *&h_pin_ref() { return h_pin_lane[lane()]; }
    int pin(size_t words) {
        uint64_t *&hp = h_pin_lane[lane()];
        size_t &hw = h_pin_words_lane[lane()];
        if (words <= hw) return LF_OK;
        if (hp) (void)hipHostFree(hp);
        hp = nullptr; hw = 0;
        if (words < pin_min_words) words = pin_min_words;
        if (hipHostMalloc((void **)&hp, words * 8) != hipSuccess) return LF_ERR_HIP;
        hw = words;
        return LF_OK;
    }
    uint64_t *round_out() {
        uint64_t *&p = h_round[lane()];
        if (!p && hipHostMalloc((void **)&p, round_out_bytes, hipHostMallocMapped) != hipSuccess) p = nullptr;
        return p;
    }
    // ---- device-resident callers (the _dev entry points): per lane, the device word the checked relayout raises on an input word >= p and the pinned word it is
    // copied to.  The copy is enqueued in front of a synchronise the call performs anyway (lf_ring_host.h, DevIo)
    uint32_t *h_flag_lane[LF_NLANES] = {nullptr, nullptr, nullptr};
    int dev_flag(uint32_t **dev, uint32_t **host) {
        uint32_t *&hf = h_flag_lane[lane()];
        if (!hf && hipHostMalloc((void **)&hf, 64) != hipSuccess) { hf = nullptr; return LF_ERR_HIP; }
        *host = hf;
        return tbuf("dev_io_flag", 16, dev);
    }
    // ---- timed launches: tag 0 = fold round kernels, 1 = ajtai, 10+i = phase i -------------------------------------------------------------------------
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<int, size_t>> ev_tags;  // (tag, event index)
    size_t ev_begin(int tag) {
        std::lock_guard<std::mutex> g(ev_mu);
        if (ev_used == ev_pool.size()) {
            EvPair e;
            (void)hipEventCreate(&e.a);
            (void)hipEventCreate(&e.b);
            ev_pool.push_back(e);
        }
        size_t i = ev_used++;
        (void)hipEventRecord(ev_pool[i].a, stream());
        ev_tags.push_back({tag, i});
        return i;
    }
    void ev_end(size_t i) {
        if (i == (size_t)-1) return;
        std::lock_guard<std::mutex> g(ev_mu);
        (void)hipEventRecord(ev_pool[i].b, stream());
    }
    void ev_reset() {
        ev_used = 0;
        ev_tags.clear();
    }
    void ev_collect() {
        (void)hipStreamSynchronize(st_lane[0]);
        (void)hipStreamSynchronize(st_lane[1]);
        k_fold_ms = k_ajtai_ms = 0;
        k_fold_n = k_ajtai_n = 0;
        for (int i = 0; i < LF_N_PHASES; i++) phase_ms[i] = 0;
        for (auto &tg : ev_tags) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev_pool[tg.second].a, ev_pool[tg.second].b);
            if (tg.first == 0) { k_fold_ms += ms; k_fold_n++; }
            else if (tg.first == 1) { k_ajtai_ms += ms; k_ajtai_n++; }
            else if (tg.first >= 10 && tg.first < 10 + LF_N_PHASES) phase_ms[tg.first - 10] += ms;
        }
        phase_ms[6] = (float)host_tr_ms;
    }
    // a sharded rank keeps columns [*col0, *col0 + *cnt) of an n-column matrix
    int shard_columns(size_t n_cols, size_t *col0, size_t *cnt) const {
        if (n_cols % (size_t)sh_world) return LF_ERR_UNSUPPORTED;
        *cnt = n_cols / sh_world;
        *col0 = *cnt * sh_rank;
        return LF_OK;
    }
    // the two prover lanes: lane 1 carries the critical chain of a fold step (two commits back to back); its kernels get dispatch priority over lane 0's
    // latency-bound linearization, which has slack
    int create_lane_streams() {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&st_lane[0], hipStreamDefault, least) != hipSuccess ||
            hipStreamCreateWithPriority(&st_lane[1], hipStreamDefault, greatest) != hipSuccess) return LF_ERR_HIP;
        return LF_OK;
    }
    int sync_lanes() {
        HIPCHK(hipStreamSynchronize(st_lane[0]));
        HIPCHK(hipStreamSynchronize(st_lane[1]));
        return LF_OK;
    }
    void drop_matrix() {   // the context holds no matrix afterwards
        if (dAb) (void)hipFree(dAb);
        setup_gen++;
        dAb = nullptr;
        A_loaded = false;
        kappa = i8_nch = i8_kc = 0;
        nA = nA_total = A_col0 = 0;
    }
    virtual ~CtxCoreBase() {}

protected:
    CtxCoreBase(size_t pin_min, size_t round_bytes) : pin_min_words(pin_min), round_out_bytes(round_bytes) {}
    const size_t pin_min_words, round_out_bytes;
    // everything above that lives on the device or in pinned memory (the streams are synchronised by the caller); the streams themselves last
    void release_base() {
        for (auto &kv : bufs) kv.second.release();
        drop_matrix();
        for (int l = 0; l < LF_NLANES; l++) {
            if (h_pin_lane[l]) (void)hipHostFree(h_pin_lane[l]);
            if (h_round[l]) (void)hipHostFree(h_round[l]);
            if (h_flag_lane[l]) (void)hipHostFree(h_flag_lane[l]);
            h_pin_lane[l] = h_round[l] = nullptr;
            h_flag_lane[l] = nullptr;
        }
        for (auto &e : ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
        ev_pool.clear();
        for (int l = 0; l < 2; l++)
            if (ev_prep[l]) (void)hipEventDestroy(ev_prep[l]);
        for (int l = 0; l < LF_NLANES; l++)
            if (st_lane[l]) (void)hipStreamDestroy(st_lane[l]);
    }
};

// W: the device word of the ring (canonical uint64_t on Goldilocks, centred Montgomery int32 on BabyBear)
template <class W>
struct CtxCore : CtxCoreBase {
    W *d_icrt = nullptr;          // the inverse CRT map, dense [RE][RE]
    W *d_icrt_sp_val = nullptr;   // its rows in compressed form ([RE][8] values / columns), null when a row has more than 8 entries
    uint32_t *d_icrt_sp_col = nullptr;
    std::vector<W *> d_val, d_valT;
    const W *vs_eq = nullptr;
    // the external basis of the extension field (lf_set_ext_basis) as the basis-changing relayout kernels take it: T and T^-1, row-major tau x tau, in the ring's
    // device word form, refreshed by every lf_set_ext_basis.  xb_on false (the identity, the default): the plain relayout kernels run
    bool xb_on = false;
    W xb_T[81] = {}, xb_Ti[81] = {};
    void free_ccs() {
        for (auto q : d_rowptr) (void)hipFree(q);
        for (auto q : d_col) (void)hipFree(q);
        for (auto q : d_val) (void)hipFree(q);
        for (auto q : d_colptr) (void)hipFree(q);
        for (auto q : d_rowidx) (void)hipFree(q);
        for (auto q : d_valT) (void)hipFree(q);
        for (auto q : d_spmvt_plan)
            if (q) (void)hipFree(q);
        d_rowptr.clear(); d_col.clear(); d_val.clear(); d_colptr.clear(); d_rowidx.clear(); d_valT.clear();
        d_spmvt_plan.clear(); spmvt_items.clear(); spmvt_cols.clear();
        have_ccs = false;
        setup_gen++;
    }
    // release everything the core owns (both lanes' streams are idle)
    void release_core() {
        free_ccs();
        if (d_icrt) (void)hipFree(d_icrt);
        if (d_icrt_sp_val) { (void)hipFree(d_icrt_sp_val); (void)hipFree(d_icrt_sp_col); }
        d_icrt = d_icrt_sp_val = nullptr;
        d_icrt_sp_col = nullptr;
        release_base();
    }

protected:
    using CtxCoreBase::CtxCoreBase;
};

// host time spent in the transcript (phase 6 of lf_last_phase_ms): one scope = one addition
struct HostTimer {
    double &acc;
    std::chrono::steady_clock::time_point t0;
    explicit HostTimer(CtxCoreBase *c) : acc(c->host_tr_ms), t0(std::chrono::steady_clock::now()) {}
    ~HostTimer() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
