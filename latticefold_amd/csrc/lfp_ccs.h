// lfp_ccs.h -- the shape of a committed CCS instance (include/lfplus.h lfplus_ccs): the refusals that lfplus_ccs_linearize, lfplus_ccs_verify and
// lfplus_ccs_check share, in the order the header states them, and the classification of the coefficients for the kernels (lfp_kernels.h CcsDesc)
#pragma once
#include <cstring>
#include <string>
#include "lfp_ctx.h"

// LFPLUS_OK: *deg = d = max |S_i| and `d` is the kernels' descriptor.  `c` may be NULL (the host-only verifier has no context to leave a message in)
static inline int lfp_ccs_shape(lfplus_ctx *c, const char *who, const lfplus_ccs *s, lfp::CcsDesc &d, u32 *deg) {
    const std::string w(who);
    if (!s || !s->S_off || !s->S_idx || !s->c) return fail(c, LFPLUS_E_ARG, w + ": null argument");
    if (s->t < 1 || s->t > 8 || s->q < 1 || s->q > 8) return fail(c, LFPLUS_E_ARG, w + ": outside the envelope (1 <= t <= 8, 1 <= q <= 8)");
    if (s->S_off[0] != 0) return fail(c, LFPLUS_E_ARG, w + ": S_off must start at 0");
    u32 dmax = 0;
    for (u32 i = 0; i < s->q; i++) {      // (entry i + 1 is read only while everything before it is in range: nothing beyond 8 x 7 indices is ever named)
        if (s->S_off[i + 1] <= s->S_off[i]) return fail(c, LFPLUS_E_ARG, w + ": S_off is not strictly increasing (every multiset has at least one index)");
        const u32 len = s->S_off[i + 1] - s->S_off[i];
        if (len > 7) return fail(c, LFPLUS_E_ARG, w + ": a multiset has more than 7 indices (d <= 7)");
        if (len > dmax) dmax = len;
    }
    if (s->S_off[s->q] > 16) return fail(c, LFPLUS_E_ARG, w + ": more than 16 indices in all (S_off[q] <= 16)");
    for (u32 k = 0; k < s->S_off[s->q]; k++)
        if (s->S_idx[k] >= s->t) return fail(c, LFPLUS_E_ARG, w + ": matrix index " + std::to_string(s->S_idx[k]) + " >= t");
    if (!canonical(s->c, (size_t)s->q * 16)) return fail(c, LFPLUS_E_ARG, w + ": non-canonical coefficient word");
    memset(&d, 0, sizeof(d));
    d.t = s->t; d.q = s->q;
    for (u32 i = 0; i < s->q; i++) {
        const u64 *cw = s->c + (size_t)i * 16;
        bool tail0 = true;
        for (int j = 1; j < 16; j++) tail0 = tail0 && cw[j] == 0;
        const u32 len = s->S_off[i + 1] - s->S_off[i];
        const u32 cls = !tail0 ? lfp::CCS_GENERAL : cw[0] == 0 ? lfp::CCS_ZERO : cw[0] == 1 ? lfp::CCS_ONE : cw[0] == lfp::P - 1 ? lfp::CCS_MINUS_ONE : lfp::CCS_CONST;
        d.cls[i] = (uint8_t)cls;
        d.len[i] = (uint8_t)len;
        d.lev[i] = (uint8_t)(cls == lfp::CCS_ZERO ? 0 : len + (cls == lfp::CCS_GENERAL ? 1 : 0));
        if (cls == lfp::CCS_CONST) d.cst[i] = (u64)((((unsigned __int128)cw[0]) << 64) % lfp::P);
        for (u32 k = 0; k < len; k++) d.op[i][k] = (uint8_t)s->S_idx[s->S_off[i] + k];
        if (d.lev[i] >= 2) d.slot[i] = (uint8_t)d.nslots++;
        if (d.lev[i] > d.maxlev) d.maxlev = d.lev[i];
    }
    if (deg) *deg = dmax;
    return LFPLUS_OK;
}
