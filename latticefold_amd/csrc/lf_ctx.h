// lf_ctx.h -- internal to the Goldilocks backend's host side (lf_capi.cpp, lf_prove.cpp, lf_fold.cpp): the context (streams, lane worker, device arena, event
// timeline, resident matrices and tables), the transcript handle and the helpers the three translation units share.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <future>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/lfhip.h"
#include "bb_capi.h"
#include "lf_ctx_core.h"
#include "lf_common.h"
#include "lf_dist.h"
#include "lf_kernels.h"
#include "lf_live_rows.h"
#include "lf_sb.h"
#include "lf_verify.h"

using namespace lf;

namespace lf {
void launch_fix_many(const DevCrt &t, const u64 *in, size_t ld_in, u64 *out, size_t ld_out, size_t n_in, u32 rows3, Fq3Const r, hipStream_t s);
}

#include <stdio.h>
#include <stdlib.h>
static bool lf_trace_on() { static int v = -1; if (v < 0) v = getenv("LF_TRACE") ? 1 : 0; return v == 1; }
#define LF_TRACE(c, msg)                                                              \
    do {                                                                              \
        if (lf_trace_on()) {                                                          \
            hipError_t e_ = hipStreamSynchronize((c)->stream());                            \
            fprintf(stderr, "[lf] %s:%d %s -> %s\n", __func__, __LINE__, msg, hipGetErrorString(e_)); \
            fflush(stderr);                                                           \
        }                                                                             \
    } while (0)

inline thread_local int t_lane = 0;  // 0 = caller thread, 1 = helper thread running the left decomposition, 2 = ingestion worker (LF_NLANES: lf_ctx_core.h)

struct lf_transcript {
    Transcript t;
    lfbb::BbTranscript *bb = nullptr;   // BabyBear transcripts live here (ring 1); t is unused then
    lf_transcript() {}
    lf_transcript(const lf_transcript &o) : t(o.t), bb(o.bb ? new lfbb::BbTranscript(*o.bb) : nullptr) {}
    ~lf_transcript() { delete bb; }
};

// wall-clock timeline of the calling thread (LF_TIMELINE=1): printed at the end of lf_fold_step
struct Timeline {
    bool on;
    std::chrono::steady_clock::time_point t0;
    std::vector<std::pair<const char *, double>> marks, marks1;   // marks1: the helper lane's thread ("L1: ..."), merged by time at the end of the step
    Timeline() : on(getenv("LF_TIMELINE") != nullptr), t0(std::chrono::steady_clock::now()) { marks1.reserve(32); }
    void mark(const char *what) {   // always recorded (lf_last_timeline); printed only with LF_TIMELINE
        marks.push_back({what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()});
    }
    void mark1(const char *what) { marks1.push_back({what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()}); }
    void merge() {
        marks.insert(marks.end(), marks1.begin(), marks1.end());
        marks1.clear();
        std::stable_sort(marks.begin(), marks.end(), [](const std::pair<const char *, double> &a, const std::pair<const char *, double> &b) { return a.second < b.second; });
    }
    void dump() {
        if (!on) return;
        double prev = 0;
        for (auto &m : marks) { fprintf(stderr, "[timeline] %-28s at %8.3f ms  (+%7.3f)\n", m.first, m.second, m.second - prev); prev = m.second; }
    }
};
inline thread_local Timeline *t_tl = nullptr;
#define TL_MARK(x) do { if (t_tl) t_tl->mark(x); } while (0)
// "<what> <round>" as a mark: the marks keep pointers, so the formatted names are interned for the life of the library
inline const char *tl_round_name(const char *what, unsigned round) {
    static std::mutex mu;
    static std::set<std::string> names;
    char nm[32];
    snprintf(nm, sizeof nm, "%s %u", what, round);
    std::lock_guard<std::mutex> g(mu);
    return names.insert(nm).first->c_str();
}
#define TL_MARK_ROUND(what, round) do { if (t_tl) t_tl->mark(tl_round_name(what, round)); } while (0)

static const char *PHASE_NAMES[LF_N_PHASES] = {"linearization", "decomp_crt_commit", "decomp_evals", "fold_prepare",
                                                "fold_sumcheck", "fold_finish", "host_transcript", "total"};

// The helper lane of a fold step: ONE thread per context, created at the first step and parked on a condition variable between steps
// (a std::async thread per step cost a thread creation + join every 7-30 ms).
struct LaneWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = false, stop = false;
    int rc = 0;
    void loop() {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return has_job || stop; });
            if (stop) return;
            std::function<int()> j = std::move(job);
            has_job = false;
            lk.unlock();
            int r = j();
            lk.lock();
            rc = r;
            done = true;
            cv.notify_all();
        }
    }
    void submit(std::function<int()> j) {
        std::unique_lock<std::mutex> lk(m);
        if (!th.joinable()) th = std::thread([this] { loop(); });
        job = std::move(j);
        has_job = true;
        done = false;
        cv.notify_all();
    }
    int wait() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return done; });
        return rc;
    }
    ~LaneWorker() {
        {
            std::unique_lock<std::mutex> lk(m);
            stop = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

struct lf_ctx : CtxCore<u64> {
    lf_ctx() : CtxCore<u64>(8192, 2 * 9 * 24 * sizeof(u64)) {}   // round_out: two messages of up to 9 evaluations x 24 words: the wide linearization round writes
                                                                  // d + 2 <= 9 (k_reduce_rows of launch_lin_round_wide), the fold rounds write their G part at word 120
    int lane() const override { return t_lane; }
    lfbb::BbCtx *bb = nullptr;   // BabyBearRingNTT backend (ring 1): every entry point forwards to it
    ExtBasis xb;          // external coordinate basis of F_{p^tau} (lf_set_ext_basis); identity by default
    hipStream_t &st_io = st_lane[2];   // lane 2: witness ingestion next to a running fold step (lf_witness_from_w_ccs_begin), lowest priority; own buffers ("lane2:" names)
    std::mutex io_mu;              // one ingestion at a time per context
    std::atomic<int> io_jobs{0};   // ingestion jobs whose worker has not finished (lf_ctx_destroy waits for them)
    // the core of whichever backend this handle drives (the external-basis marshalling and the read-outs are ring-agnostic)
    inline CtxCoreBase &core_any();
    bool have_ccs_any() { return core_any().have_ccs; }
    const lf_params &params_any() { return core_any().P; }
    size_t n_any() { return core_any().n; }
    size_t m_any() { return core_any().m; }
    size_t N_any() { return core_any().N; }
    HostRing ring;
    DevCrt dcrt;
    // the z_k build's int8 matrix (lf_zk_i8.hip) of dcrt for the base of the loaded parameters: built at the first z_k build that can use it, on the calling
    // lane's stream (set-up: one synchronisation), and again after install_tables or a change of B
    ZkI8 zk_i8;
    std::mutex zk_mu;    // (either lane may be the first to ask)
    int zk_i8_get(u64 B, const ZkI8 **out) {
        std::lock_guard<std::mutex> g(zk_mu);
        if (zk_i8.state == 0 || zk_i8.B != B)
            if (zk_i8_prepare(dcrt, B, &zk_i8, stream()) != 0) return LF_ERR_HIP;
        *out = zk_i8.state == 1 ? &zk_i8 : nullptr;
        return LF_OK;
    }
    LaneWorker lane1;
    int agreed_two_lanes = -1;       // lf_dist_init's handshake: the schedule ALL ranks agreed on (1 threaded / 0 one thread); -1 = no handshake ran (host transports, model)
    bool two_lanes_ok = false;       // the transport's two channels have been seen working concurrently (lf_dist_init's handshake; two host callbacks): a sharded
                                     // step then runs the threaded two-lane schedule unless LF_SHARD_TWO_LANES=0
    // exchange layer, one per prover lane: the two lanes of a fold step exchange concurrently (lane 0: linearization rounds and right evaluations,
    // lane 1: commits and left evaluations) and collectives of ONE communicator must be issued in the same order on every rank.  Lane 2 never exchanges
    lfdist::Comm comm[2];
    lfdist::Comm &cm() { assert(t_lane < 2); return comm[t_lane]; }
    bool ccs_general = false;   // some constraint matrix has more than ~1.5 entries per (non-empty) row: M z runs on k_spmv_rows (whole-element gathers from an element-major z)
    size_t live_rows = 0;       // 1 + the last row with an entry in any constraint matrix (lf_live_rows.h; fixed at lf_ccs_load): the rows behind it are zeros of every M_j z
    // the padded live prefix the linearization and the G tables of this call work on (the switches are read per call); sharded contexts keep whole tables
    lflive::Plan live_plan() const {
        if (tn.no_live_rows || sh_world > 1) return lflive::plan(m, m, 0, 0);
        return tn.live_rows_low ? lflive::plan(m, live_rows, lflive::GRANULE_LOW, lflive::MIN_M_LOW) : lflive::plan(m, live_rows, lflive::GRANULE, lflive::MIN_M);
    }
    // sharded step: the columns of z this rank's row slice of the constraint matrices refers to (shard_col_range; (size_t)-1 = not computed)
    size_t shc_r0 = (size_t)-1, shc_rcnt = 0, shc_lo = 0, shc_hi = 0;
    LinCombDesc desc{};
    std::vector<std::pair<const char *, double>> tl_marks;   // wall-clock marks of the last fold step (lf_last_timeline)
    // bit-plane forms of the two witnesses of the running fold step (lf_sv_rounds.h), enqueued on the helper lane's stream before anything else
    const lf_witness *bits_wit[2] = {nullptr, nullptr};
    u32 *bits_ptr[2] = {nullptr, nullptr};
    hipEvent_t bits_ev[2] = {nullptr, nullptr};
    hipEvent_t ev_yR = nullptr, ev_yL = nullptr;  // the right / left commit's results are in h_pin2 (second / first half)
    u64 *h_pin2 = nullptr;
    size_t h_pin2_words = 0;
    int pin2(size_t words) {
        if (words <= h_pin2_words) return LF_OK;
        if (h_pin2) (void)hipHostFree(h_pin2);
        h_pin2 = nullptr; h_pin2_words = 0;
        if (hipHostMalloc((void **)&h_pin2, words * 8) != hipSuccess) return LF_ERR_HIP;
        h_pin2_words = words;
        return LF_OK;
    }
    // linearization: the pass of the v_s evaluations over the witness starts on this stream while the last sumcheck rounds are still running (VsSplit)
    hipStream_t st_aux = nullptr;
    hipEvent_t ev_aux = nullptr;
    u64 *h_aux = nullptr;   // pinned, 1 KB: the known part of the point
    unsigned lin_split_rounds = 0;   // rounds of the last linearization sumcheck that ran in the split eq form (run_lin_sumcheck)
    unsigned lin_live_rounds = 0;    // ... and those that ran over a live prefix of their tables only (lf_live_rows.h)

    // Small host-to-device uploads inside a step (challenge powers, look-up tables, evaluation points) go through a pinned ring per lane:
    // the copy is truly asynchronous and the caller's stack / vector buffer is free at once -- no stream synchronisation per upload.
    unsigned char *stage[LF_NLANES] = {nullptr, nullptr, nullptr};
    size_t stage_off[LF_NLANES] = {0, 0, 0};
    static constexpr size_t STAGE_BYTES = (size_t)1 << 20;
    int h2d_small(void *dst, const void *src, size_t bytes) {
        unsigned char *&ring = stage[t_lane];
        if (!ring && hipHostMalloc((void **)&ring, STAGE_BYTES, hipHostMallocDefault) != hipSuccess) { ring = nullptr; return LF_ERR_HIP; }
        const size_t need = (bytes + 63) & ~(size_t)63;
        if (need > STAGE_BYTES) {   // not small: plain blocking copy
            HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream()));
            HIPCHK(hipStreamSynchronize(stream()));
            return LF_OK;
        }
        if (stage_off[t_lane] + need > STAGE_BYTES) {   // wrap: everything staged so far must have left the ring
            HIPCHK(hipStreamSynchronize(stream()));
            stage_off[t_lane] = 0;
        }
        unsigned char *slot = ring + stage_off[t_lane];
        stage_off[t_lane] += need;
        memcpy(slot, src, bytes);
        HIPCHK(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, stream()));
        return LF_OK;
    }
    // persistent sumcheck tail (k_fold_tail): host-mapped mailbox + device scratch, created on first use
    TailMail *tail_mail = nullptr;
    u32 *tail_counters = nullptr;      // device, TAIL_MAX_ROUNDS u32 (zeroed once; self-resetting) followed by dev_chal
    u64 *tail_dev_chal = nullptr;
    u32 tail_epoch = 0;
    int num_cus = 0;
    int tail_setup() {
        if (tail_mail) return LF_OK;
        hipDeviceProp_t pr;
        HIPCHK(hipGetDeviceProperties(&pr, device));
        num_cus = pr.multiProcessorCount;
        void *d = nullptr;
        HIPCHK(lf_dev_malloc(&d, 4096));
        HIPCHK(hipMemset(d, 0, 4096));
        tail_counters = (u32 *)d;
        tail_dev_chal = (u64 *)((char *)d + 1024);
        HIPCHK(hipHostMalloc((void **)&tail_mail, sizeof(TailMail), hipHostMallocMapped | hipHostMallocCoherent));   // fine-grained: the kernel and this thread talk through it while the kernel runs
        memset(tail_mail, 0, sizeof(TailMail));
        return LF_OK;
    }
    u64 *d_poseidon = nullptr;   // device copy of the Poseidon constants: ark [720] then mds [576]
    int poseidon_setup() {
        if (d_poseidon) return LF_OK;
        const u64 *a, *m;
        Transcript::params(&a, &m);
        HIPCHK(lf_dev_malloc(&d_poseidon, (720 + 576) * 8));
        HIPCHK(hipMemcpy(d_poseidon, a, 720 * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_poseidon + 720, m, 576 * 8, hipMemcpyHostToDevice));
        return LF_OK;
    }
    hipEvent_t ev_theta = nullptr;
    hipEvent_t ev_block = nullptr;   // hipEventBlockingSync: lane 1 (long waits) yields its CPU instead of spinning
    int lane_sync() {
        if (t_lane == 1 && ev_block) {
            HIPCHK(hipEventRecord(ev_block, st_lane[1]));
            HIPCHK(hipEventSynchronize(ev_block));
            return LF_OK;
        }
        HIPCHK(hipStreamSynchronize(stream()));
        return LF_OK;
    }
};
inline CtxCoreBase &lf_ctx::core_any() { return bb ? bb->core() : *this; }


// ---- shared between lf_capi.cpp / lf_prove.cpp / lf_fold.cpp (hidden: not part of the ABI) -------------------------------------------------------
#pragma GCC visibility push(hidden)
Fq3Const f3c(Fq3 a);
bool shard_keep(const lf_ctx *c, int kind, size_t n);
int build_eq_dev(lf_ctx *c, const Fq3 *pt, u32 nv, u64 *eq_dev);
int exchange_modsum_dev(lf_ctx *c, u64 *inout_dev, size_t words);
int down_small(lf_ctx *c, const u64 *dsrc, size_t words, u64 *host);
void shard_slice(const lf_ctx *c, size_t n, size_t *i0, size_t *cnt);
struct GatherPart { const u64 *src; size_t src_ld; u64 *dst; size_t planes; };
int shard_col_range(lf_ctx *c, size_t r0, size_t rcnt, size_t *lo, size_t *hi);
int gather_slices(lf_ctx *c, u64 *buf, size_t planes, size_t n);
struct SideState {
    const int32_t *planes = nullptr;
    u64 *z = nullptr;       // [K][24][n]
    u64 *eq_r = nullptr;    // [3][m]
    std::vector<u64> lcccs;  // K flat LCCCS (host)
    // z_k (and x_s in the proof) may be built ahead of the evaluation point by the other lane (decompose_prepare_z): 1 = published
    // (z, x_s valid once z_ev has completed), -1 = that lane failed, 0 = nobody built it yet
    std::atomic<int> z_state{0};
    hipEvent_t z_ev = nullptr;
    const unsigned char *D = nullptr;   // small-base path (b > 2, lf_sb.h): the K digit planes of the side's witness, [K][24][sb_ld(N)]
    u32 *sv_bits = nullptr;  // bit-plane form of the witness planes for the GEMM rounds of the folding sumcheck (lf_sv_rounds.h), if built ahead
    ~SideState() { if (z_ev) (void)hipEventDestroy(z_ev); }
};
int gather_parts(lf_ctx *c, const GatherPart *parts, int np, size_t lcl);
// External basis at the ABI.  What is SMALL is converted here, on the host, by the wrapper at the head of an entry point (XB below): instances, proofs,
// commitments, challenges and points, sumcheck messages, the CSR values of lf_ccs_load, and the transcript through its basis hook.  The O(n) ARRAYS in NTT form
// are converted on the device, by the relayout kernels that move them between the caller's AoS words and the planes (up_ring / down_ring, lf_ring_host.h): the
// wrapper of such an entry point -- host-pointer call or _dev twin -- opens XB with arrays = true, and the staging helpers convert an array of Form::ntt while
// t_xb_arrays is up.  Everything a wrapper calls runs with t_xb_active up, so no inner entry point converts again; lf_fold_step and the sub-provers open XB
// without arrays, so nothing they stage is converted either.
inline thread_local bool t_xb_active = false;   // external-basis conversion in progress on this thread
inline thread_local bool t_xb_arrays = false;   // ... and the NTT-form arrays of the running entry point change basis in its relayout kernels
struct XB {
    lf_ctx *c;
    size_t RE, TAU;
    std::vector<std::unique_ptr<std::vector<u64>>> keep;
    lf_transcript *tr = nullptr;
    explicit XB(lf_ctx *cc, bool arrays = false) : c(cc), RE((size_t)lf_ring_words(lf_ctx_ring(cc))), TAU((size_t)lf_ring_tau(lf_ctx_ring(cc))) {
        t_xb_active = true;
        t_xb_arrays = arrays;
    }
    ~XB() {
        t_xb_active = false;
        t_xb_arrays = false;
        if (tr) { tr->t.set_basis(nullptr, nullptr); if (tr->bb) tr->bb->set_basis(nullptr, nullptr); }
    }
    const u64 *ring_in(const u64 *p, size_t elems) {   // a few NTT-form ring elements, external -> internal (copy)
        if (!p) return p;
        keep.emplace_back(new std::vector<u64>(p, p + elems * RE));
        c->xb.to_int(keep.back()->data(), elems * 8);
        return keep.back()->data();
    }
    const u64 *ext_in(const u64 *p, size_t n) {        // F_{p^tau} elements (tau words each)
        if (!p) return p;
        keep.emplace_back(new std::vector<u64>(p, p + n * TAU));
        c->xb.to_int(keep.back()->data(), n);
        return keep.back()->data();
    }
    void ring_out(u64 *p, size_t elems) { if (p) c->xb.to_ext(p, elems * 8); }
    void ext_out(u64 *p, size_t n) { if (p) c->xb.to_ext(p, n); }
    void transcript(lf_transcript *t) {
        tr = t;
        if (t->bb) t->bb->set_basis(c->xb.T, c->xb.Ti);
        else t->t.set_basis(c->xb.T, c->xb.Ti);
    }
};
#define LF_XB(c) ((c) && (c)->xb.on && !t_xb_active)
// the whole wrapper of an entry point whose only basis-dependent arguments are O(n) arrays (host-pointer call or _dev twin): nothing is copied or converted on
// the host, the relayout kernels of the body change the basis
struct XbArrays {
    const bool set;
    explicit XbArrays(lf_ctx *c) : set(LF_XB(c)) { if (set) t_xb_active = t_xb_arrays = true; }
    ~XbArrays() { if (set) t_xb_active = t_xb_arrays = false; }
};
int fold_impl(lf_ctx *c, Transcript &tr, SideState *S /* [2] */, u64 *lcccs_out, lf_witness **w_out, u64 *proof);
int commit_download(lf_ctx *c, const u64 *dev, size_t words, u64 *host);
// small-base path: the NP part commitments y_k = A f_k of the digit planes D [NP][24][ldn] (lf_sb.h) in ONE pass over A -> out_dev [NP][kappa][24] NTT form
int commit_parts_i8g(lf_ctx *c, const unsigned char *D, size_t ldn, u32 NP, u64 *out_dev);
// the digit planes of a witness, cut on the calling lane's stream into the buffer `name`
int sb_cut_parts(lf_ctx *c, const lf_witness *wit, const char *name, const unsigned char **D);
int fold_impl_sb(lf_ctx *c, Transcript &tr, SideState *S /* [2] */, u64 *lcccs_out, lf_witness **w_out, u64 *proof);
// One run of the folding prover: the state its stages share, and the stages that are the same code for b = 2 (lf_fold.cpp, which defines them) and for the
// small bases (lf_fold_sb.cpp).  A stage queues on the stream it is given: the streams a path uses are that path's schedule.
struct FoldStep {
    lf_ctx *c;
    Transcript &tr;
    SideState *S;   // [2]
    u64 *proof;     // the s round messages, theta, eta
    const lf_params &P;
    const size_t m, n, N;
    const u32 K, K2, deg;
    const GoldV hv;
    std::vector<Fq3> alpha, zeta, mu, beta, pt;
    Fq3Const *d_mu = nullptr, *d_ap = nullptr, *d_zp = nullptr;   // challenge powers x^{j+1}
    u64 *G[2] = {nullptr, nullptr}, *eqb = nullptr, *zz = nullptr;
    FoldRoundArgs a;                       // the five special tables of the current round
    u64 *T5[2] = {nullptr, nullptr};       // ... fixed ping-pong, 57 planes per buffer
    const u64 *curF = nullptr;             // the materialised f-hat tables (null while they are virtual)
    size_t ldF = 0;
    u64 *eq0 = nullptr, *q = nullptr, *dpart = nullptr, *d_theta = nullptr, *d_eta = nullptr;
    FoldStep(lf_ctx *c, Transcript &tr, SideState *S, u64 *proof);
    u64 *msg(u32 round) const { return proof + (size_t)(round - 1) * (deg + 1) * 24; }
    u64 *theta() const { return proof + (size_t)P.s * (deg + 1) * 24; }
    u64 *eta() const { return theta() + (size_t)K2 * 72; }
    // prepare
    int powers_alpha_zeta();
    int powers_mu();
    int prepare_buffers();
    int side_mz(int sd, hipStream_t st, u64 *zb, const char *zaos_name, size_t zc_lo, size_t zc_hi, size_t g_r0 = 0, size_t g_rcnt = (size_t)-1);
    // rounds
    void first_tables();
    void fix_special(u32 round, Fq3Const r, u64 *dst, hipStream_t sg);
    void set_tables(u64 *dst, size_t nn);
    // evaluations, finish
    int eval_buffers(bool q_words = true);
    int gather_q(hipStream_t s1f);
    int finish(u64 *lcccs_out, lf_witness **w_out, const std::function<int(const std::vector<int8_t> &rho8, int8_t *d_rho, int32_t *npl)> &fold_witness);
};
int sb_fold_round_abi(lf_ctx *c, const u64 *t5, const u64 *F, size_t n, const Fq3Const *d_mu, u64 *evals_out);
int dot_batch_dev(lf_ctx *c, const u64 *X, size_t ldx, u32 na, const u64 *Y, size_t ldy, u32 nb, size_t n, u64 *dpart, u64 *od, hipStream_t st = nullptr,
                         const char *tag = "", unsigned char *yb_pre = nullptr);
bool q_pack_takes(lf_ctx *c, const u64 *X, size_t ldx, u32 na);
int q_pack_dev(lf_ctx *c, const u64 *X, const u64 *eq, unsigned char **yb);
int coef_eval_dev(lf_ctx *c, const int32_t *planes, size_t n, const u64 *eq, size_t ldeq, u32 K, int mode_bits, u64 *partial, u64 *od, size_t ldp,
                         const lf_witness *wit = nullptr);
int lin_tail_rounds(lf_ctx *c, Transcript &tr, const u64 *cur, const u64 *cure, size_t n, u64 *tout, u64 *partial, u32 round, Fq3 *point,
                           u64 *msgs, u32 deg, const std::function<void(u32)> *after_round);
// z tables [K][24][n] = heads (l + 1 elements per table) || the recomposed witness columns [w0, w0 + wcnt) (lf_prove.cpp)
int build_z(lf_ctx *c, const int32_t *planes, u32 K, int mode_bits, const u64 *heads, u64 *z, size_t w0 = 0, size_t wcnt = (size_t)-1,
            const unsigned char *D = nullptr /* small-base path: the digit planes the K parts come from (lf_sb.h) */);
#pragma GCC visibility pop
