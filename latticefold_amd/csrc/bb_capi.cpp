// bb_capi.cpp -- BabyBearRingNTT backend of the C ABI, part 1: context, ring tables, staging, the component entry points (CRT, decomposition, Ajtai
// commitments, eq tables, MLE evaluations, SpMV), constraint-system load, device-resident witnesses, timing read-outs and the host verifier.  The provers are
// in bb_prove.cpp.
#include "lf_ring_host.h"

namespace lfbb {

// ---------------------------------------------------------------------------------------------------------------
static int install_tables(C *c, u64 nonres, const u64 *y) {
    static thread_local BbTables T;
    if (bb_build_tables(nonres, y, T) != 0) return LF_ERR_BAD_TABLES;
    c->ring.T = T;
    c->dev = make_dev_bb(T);
    return ring_ops<BbRing>::install_icrt(c, &T.icrt[0][0]);
}
int BbCtx::create(BbCtx **out, lf_ctx *owner, int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0 || device < 0 || device >= cnt) return LF_ERR_HIP;
    HIPCHK(hipSetDevice(device));
    C *c = new C();
    c->owner = owner;
    c->device = device;
    if (c->create_lane_streams() != LF_OK) { delete c; return LF_ERR_HIP; }
    c->arena_words = (size_t)1 << 19;   // 4 MiB per lane
    for (int l = 0; l < 2; l++) {
        if (hipHostMalloc((void **)&c->arena[l], c->arena_words * 8) != hipSuccess) { delete c; return LF_ERR_HIP; }
        if (hipEventCreateWithFlags(&c->ev_side[l], hipEventDisableTiming) != hipSuccess) { delete c; return LF_ERR_HIP; }
    }
    for (int l = 0; l < 4; l++)
        if (hipEventCreateWithFlags(&c->ev_dec[l], hipEventDisableTiming) != hipSuccess) { delete c; return LF_ERR_HIP; }
    u64 nr, y[8 * TAU];
    bb_default_ring(&nr, y);
    int rc = install_tables(c, nr, y);
    if (rc != LF_OK) { delete c; return rc; }
    BbCtx *b = new BbCtx();
    b->p = c;
    *out = b;
    return LF_OK;
}
void BbCtx::destroy() {
    C *c = p;
    (void)hipSetDevice(c->device);
    (void)c->sync_lanes();
    c->comm.destroy();
    for (int l = 0; l < 2; l++) {
        if (c->arena[l]) (void)hipHostFree(c->arena[l]);
        if (c->ev_side[l]) (void)hipEventDestroy(c->ev_side[l]);
    }
    for (int l = 0; l < 4; l++)
        if (c->ev_dec[l]) (void)hipEventDestroy(c->ev_dec[l]);
    c->release_core();
    delete c;
    delete this;
}
CtxCoreBase &BbCtx::core() { return *p; }
int BbCtx::set_ring_tables(uint64_t nonres, const uint64_t *y) {
    std::lock_guard<std::mutex> g(p->mu);
    HIPCHK(hipSetDevice(p->device));
    RET(p->sync_lanes());
    return install_tables(p, nonres, y);
}
int BbCtx::set_sharding(int rank, int world, lf_exchange_fn cb, void *user) {
    if (world < 1 || rank < 0 || rank >= world || (world & (world - 1)) != 0 || (world > 1 && !cb)) return LF_ERR_INVALID;
    std::lock_guard<std::mutex> g(p->mu);
    if (p->A_loaded) return LF_ERR_STATE;   // choose the sharding before loading/generating the Ajtai matrix
    p->comm.destroy();
    p->comm.rank = p->sh_rank = rank; p->comm.world = p->sh_world = world; p->comm.cb = cb; p->comm.user = user;
    return LF_OK;
}
int BbCtx::dist_init(int rank, int world, const uint8_t *id128) {
    std::lock_guard<std::mutex> g(p->mu);
    if (p->A_loaded) return LF_ERR_STATE;
    HIPCHK(hipSetDevice(p->device));
    p->comm.destroy();
    RET(lfdist::rccl_init(p->comm, rank, world, id128));
    p->sh_rank = rank; p->sh_world = world;
    return LF_OK;
}
int BbCtx::get_ring_tables(uint64_t *nonres, uint64_t *y) {
    *nonres = p->ring.T.nu;
    for (int k = 0; k < 8; k++)
        for (int q = 0; q < TAU; q++) y[TAU * k + q] = p->ring.T.y[k].c[q];
    return LF_OK;
}
// small device array -> host through pinned memory (up_ring / down_ring: lf_ring_host.h)
int down_small(C *c, const u64 *dsrc, size_t words, u64 *host) {
    RET(c->pin(words));
    HIPCHK(hipMemcpyAsync(c->h_pin_ref(), dsrc, words * 8, hipMemcpyDeviceToHost, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));
    memcpy(host, c->h_pin_ref(), words * 8);
    return LF_OK;
}
// all-gather `words` canonical words from every rank and add them mod p (RCCL has no modular reduction)
int exchange_modsum(C *c, u64 *inout, size_t words) {
    if (c->sh_world <= 1) return LF_OK;
    std::vector<u64> all((size_t)c->sh_world * words);
    RET(c->comm.allgather_host(inout, all.data(), words, c->stream()));
    for (size_t w = 0; w < words; w++) {
        u64 acc = 0;
        for (int g = 0; g < c->sh_world; g++) {
            u64 v = all[(size_t)g * words + w];
            if (v >= BB_P) return LF_ERR_INVALID;
            acc = hadd(acc, v);
        }
        inout[w] = acc;
    }
    return LF_OK;
}

// ---- arithmetic self-test: operands ----------------------------------------------------------------------------------
// The kernels' bounds are bounds on the DEVICE word, the centred Montgomery word in [-H, H] (bb_field.cuh): canonical corners such as p - 1 or (p +- 1) / 2
// are words at 27 % and 13 % of H and reach neither the top of a 64-bit column nor the pre-centring of mred.  The first operand pairs therefore put every pair
// of the device-word grid below (tests/field_corners.py: EDGE_BW) into every pair of coordinate positions, followed by the saturating pairs -- a_i = +-H,
// b_j = H for j <= k and nu b_j = H for j > k, so that column k is nine terms of +-H^2 -- of nu = 2 and of the context's nu; the rest are pseudo-random.
namespace selftest_bb {
constexpr int32_t H = BB_H, R32 = (int32_t)BB_R;
constexpr int NG = 30;
const int32_t GRID[NG] = {0, 1, -1, 2, -2, H, -H, H - 1, -(H - 1), H / 2, -(H / 2), H / 2 + 1, -(H / 2 + 1), R32, -R32, 1 << 29, -(1 << 29),
                          0x3B7F7F7F, -0x3B7F7F7F, 0x3B808080, -0x3B808080, 0x007F7F7F, -0x00808080, 0x7F, -0x80, 0x80, -0x81, 0x7FFF, 0x8000, -0x8000};
inline u64 pw(u64 a, u64 e) { u64 r = 1; a %= BB_P; while (e) { if (e & 1) r = r * a % BB_P; a = a * a % BB_P; e >>= 1; } return r; }
inline u64 canon_of(int32_t w) { return (u64)((i64)w + (i64)BB_P) % BB_P * pw(BB_R, BB_P - 2) % BB_P; }   // device word -> canonical residue
void operands(u64 seed, u32 n, u64 nu, std::vector<u64> &in) {
    in.resize((size_t)n * 18);
    u64 cg[NG];
    for (int i = 0; i < NG; i++) cg[i] = canon_of(GRID[i]);
    u32 i = 0;
    for (int sh = 0; sh < TAU && i < n; sh++)
        for (int x = 0; x < NG && i < n; x++)
            for (int y = 0; y < NG && i < n; y++, i++)
                for (int q = 0; q < TAU; q++) { in[(size_t)i * 18 + q] = cg[(x + q * sh) % NG]; in[(size_t)i * 18 + 9 + q] = cg[(y + 5 * q * sh) % NG]; }
    const u64 nus[2] = {2, nu % BB_P};
    for (int v = 0; v < 2; v++) {
        const u64 hi = canon_of(H), half = nus[v] == 2 ? canon_of(H / 2) : hi * pw(nus[v], BB_P - 2) % BB_P;
        for (int sg = 0; sg < 2; sg++)
            for (int k = 0; k < TAU && i < n; k++, i++)
                for (int q = 0; q < TAU; q++) { in[(size_t)i * 18 + q] = canon_of(sg ? -H : H); in[(size_t)i * 18 + 9 + q] = q <= k ? hi : half; }
    }
    u64 s = seed * 0x9E3779B97F4A7C15ULL + 1;
    for (size_t k = (size_t)i * 18; k < in.size(); k++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        in[k] = s % BB_P;
    }
}
}  // namespace selftest_bb

int BbCtx::selftest_field(uint64_t seed, uint32_t n, uint64_t *mismatches) {
    C *c = p;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    std::vector<u64> in, out((size_t)n * 12);
    selftest_bb::operands(seed, n, c->ring.T.nu, in);
    u64 *di, *dout;
    RET(c->tbuf("io_a", in.size() * 2, (fe **)&di));
    RET(c->tbuf("io_b", out.size() * 2, (fe **)&dout));
    HIPCHK(hipMemcpyAsync(di, in.data(), in.size() * 8, hipMemcpyHostToDevice, c->stream()));
    launch_selftest(di, dout, n, c->dev.nu, c->stream());
    HIPCHK(hipMemcpyAsync(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));
    u64 bad = 0;
    for (u32 i = 0; i < n; i++) {
        H9 a = h9_load(&in[(size_t)i * 18]), b = h9_load(&in[(size_t)i * 18 + 9]);
        H9 pr = c->ring.mul9(a, b);
        for (int q = 0; q < TAU; q++) bad += out[(size_t)i * 12 + q] != pr.c[q];
        bad += out[(size_t)i * 12 + 9] != hadd(a.c[0], b.c[0]);
        bad += out[(size_t)i * 12 + 10] != hsub(a.c[0], b.c[0]);
        bad += out[(size_t)i * 12 + 11] != hmul(a.c[0], b.c[0]);
    }
    *mismatches = bad;
    return LF_OK;
}

// ---- a8/a9/a11 ---------------------------------------------------------------------------------------------------------
// no host synchronisation: constants are staged in the lane's pinned arena (valid until the next fold step)
int build_eq_async(C *c, const H9 *pt, u32 nv, fe *eq_dev) {
    E9PreC *rd;
    RET(c->tbuf("eq_point_async", 2 * 64, &rd));
    size_t words = (2 * (size_t)nv * sizeof(E9PreC) + 7) / 8;
    E9PreC *h = (E9PreC *)c->arena_alloc(words);
    if (!h) return LF_ERR_HIP;
    for (u32 i = 0; i < nv; i++) {
        h[i] = e9pre_from_h9(pt[i], c->ring.T.nu);
        H9 om;
        for (int q = 0; q < TAU; q++) om.c[q] = hsub(q == 0 ? 1 : 0, pt[i].c[q]);
        h[nv + i] = e9pre_from_h9(om, c->ring.T.nu);
    }
    HIPCHK(hipMemcpyAsync(rd, h, 2 * (size_t)nv * sizeof(E9PreC), hipMemcpyHostToDevice, c->stream()));
    launch_build_eq(c->dev, rd, rd + nv, nv, eq_dev, c->stream());
    return LF_OK;
}
int build_eq_dev(C *c, const H9 *pt, u32 nv, fe *eq_dev) {
    E9PreC *rd;
    RET(c->tbuf("eq_point", 2 * 64, &rd));
    std::vector<E9PreC> h(2 * (size_t)nv);
    for (u32 i = 0; i < nv; i++) {
        h[i] = e9pre_from_h9(pt[i], c->ring.T.nu);
        h[nv + i] = e9pre_from_h9(h9_sub(h9_one(), pt[i]), c->ring.T.nu);
    }
    HIPCHK(hipMemcpyAsync(rd, h.data(), h.size() * sizeof(E9PreC), hipMemcpyHostToDevice, c->stream()));
    HIPCHK(hipStreamSynchronize(c->stream()));
    launch_build_eq(c->dev, rd, rd + nv, nv, eq_dev, c->stream());
    return LF_OK;
}
// ---- CCS ------------------------------------------------------------------------------------------------------------------
// the envelope of lf_ccs_load on this ring (the rest is ring_ops::ccs_load)
int ccs_envelope(const lf_params *P) {
    if (P->s < 3 || P->s > 28 || P->t == 0 || P->t > 4 || P->q == 0 || P->q > 8 || P->K == 0 || P->K > 16 || P->L == 0 || P->L > 8 ||
        P->d + 1 > 4 || P->wit_len == 0)
        return LF_ERR_UNSUPPORTED;
    if (P->b != 2) return LF_ERR_UNSUPPORTED;
    if (!pow2(P->B) || P->B > (1ULL << 30)) return LF_ERR_UNSUPPORTED;
    {
        u64 half = P->B / 2;
        u32 need = 0;
        while ((half >> need) != 0) need++;
        if (need > P->K) return LF_ERR_UNSUPPORTED;
    }
    return LF_OK;
}

// ---- host-side verifier ------------------------------------------------------------------------------------------------------------
// the host ring with the default tables: what the context-free verifiers compute in
static const BbHostRing &default_host_ring() {
    static const BbHostRing *ring = [] {
        BbHostRing *g = new BbHostRing();
        u64 nr, y[8 * TAU];
        bb_default_ring(&nr, y);
        bb_build_tables(nr, y, g->T);
        return g;
    }();
    return *ring;
}
int bb_mlsumcheck_verify(BbTranscript &tr, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum, const uint64_t *msgs, uint64_t *point_out,
                         uint64_t *expected_out) {
    return lfv::mlsumcheck_verify(BbV{default_host_ring()}, tr, nvars, degree, claimed_sum, msgs, point_out, expected_out);
}
int bb_verify_host(const lf_params *p, const uint32_t *S_off, const uint32_t *S_idx, const uint64_t *c, BbTranscript &tr, const uint64_t *acc,
                   const uint64_t *cm_i, const uint64_t *proof, uint64_t *lcccs_out, int *failed_stage) {
    const BbV bv{default_host_ring()};
    lfv::Verifier<BbV> V(bv, *p, S_off, S_idx, c);
    int rc = V.verify(tr, acc, cm_i, proof, lcccs_out);
    if (failed_stage) *failed_stage = V.stage;
    return rc;
}

}  // namespace lfbb

