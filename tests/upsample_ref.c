/* upsample_ref.c -- TEST INFRASTRUCTURE: a plain C statement of what
 * mm_upsample_frames and mm_fill_pixels compute (include/mm_api.h), IEEE
 * binary32 in the order written there, built with the oracle Makefile's
 * CFLAGS (-ffp-contract=off, no fast-math).  tests/upsample_support.py binds
 * it.
 *
 * It counts what every pixel and every tap of a call met: UPREF_N_COUNTS
 * uint64 (see the enum), so that a test can tell whether its inputs made every
 * clause decide something. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../include/mm_types.h"

enum {
    UPREF_LATTICE = 0,   /* pixels: on the lattice (x and y multiples of s)              */
    UPREF_TAP_OUTSIDE,   /* taps skipped: Q outside the lattice                          */
    UPREF_TAP_ZERO,      /* taps skipped: inside, g == 0                                 */
    UPREF_REJ_ID,        /* taps skipped: id_q != id_p                                   */
    UPREF_REJ_MH,        /* ... ids equal, al_q.w != al_p.w                              */
    UPREF_REJ_NORMAL,    /* ... ids and mirror hits equal, normals' dot < 0              */
    UPREF_TAKEN,         /* taps taken                                                   */
    UPREF_HOLE_W,        /* pixels: a hole, the valid taps' weight is below w_min        */
    UPREF_HOLE_FAILED,   /* pixels: a hole, id is MM_AOV_ID_FAILED                       */
    UPREF_FROM_1,        /* pixels off the lattice interpolated from 1 tap               */
    UPREF_FROM_2,        /* ... from 2                                                   */
    UPREF_FROM_3,        /* ... from 3                                                   */
    UPREF_FROM_4,        /* ... from 4                                                   */
    UPREF_N_COUNTS
};

int upref_n_counts(void) { return UPREF_N_COUNTS; }

/* low: n_frames*lw*lh float4; nd, al: n_frames*w*h float4; id: n_frames*w*h; low_vmean: n_frames*lw*lh or NULL;
 * out: n_frames*w*h float4; weight_out, var_out: n_frames*w*h or NULL; counts: UPREF_N_COUNTS uint64, added to
 * (NULL: not kept).  Returns 0, or -1 for arguments mm_upsample_frames rejects. */
int upref_upsample(const float* low, const float* nd, const float* al, const uint32_t* id, const float* low_vmean,
                   uint32_t s, float w_min, uint32_t n_frames, uint32_t w, uint32_t h, float* out, float* weight_out,
                   float* var_out, uint64_t* counts) {
    uint64_t local[UPREF_N_COUNTS] = {0};
    uint64_t* cnt = counts ? counts : local;
    if (!low || !nd || !al || !id || !out || !w || !h || !n_frames) return -1;
    if ((s != 2 && s != 4 && s != 8) || !(w_min > 0.0f && w_min <= 1.0f) || (var_out && !low_vmean)) return -1;
    const uint32_t lw = (w + s - 1) / s, lh = (h + s - 1) / s;
    const float inv_s = 1.0f / (float)s;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t fo = (size_t)f * w * h, lo = (size_t)f * lw * lh;
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t p = fo + (size_t)y * w + x;
                float* o = out + 4 * p;
                o[0] = o[1] = o[2] = o[3] = 0.0f;  /* HOLE, until the taps say otherwise */
                if (weight_out) weight_out[p] = 0.0f;
                if (var_out) var_out[p] = 0.0f;
                const uint32_t X0 = x / s, Y0 = y / s;
                const int lattice = x == s * X0 && y == s * Y0;
                if (lattice) cnt[UPREF_LATTICE]++;
                const float a = (float)(x - s * X0) * inv_s, b = (float)(y - s * Y0) * inv_s;
                const uint32_t idp = id[p];
                if (idp == MM_AOV_ID_FAILED) { cnt[UPREF_HOLE_FAILED]++; continue; }
                const float* ndp = nd + 4 * p;
                const float mhp = al[4 * p + 3];
                float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f, G2 = 0.0f, SV = 0.0f;
                int taken = 0;
                for (int t = 0; t < 4; ++t) {
                    const uint32_t dx = t & 1, dy = t >> 1;
                    const uint32_t Qx = X0 + dx, Qy = Y0 + dy;
                    if (Qx >= lw || Qy >= lh) { cnt[UPREF_TAP_OUTSIDE]++; continue; }
                    const float g = (dx ? a : 1.0f - a) * (dy ? b : 1.0f - b);
                    if (!(g > 0.0f)) { cnt[UPREF_TAP_ZERO]++; continue; }
                    const size_t q = fo + (size_t)(s * Qy) * w + (size_t)(s * Qx);
                    const size_t lq = lo + (size_t)Qy * lw + Qx;
                    const float* ndq = nd + 4 * q;
                    if (id[q] != idp) { cnt[UPREF_REJ_ID]++; continue; }
                    if (!(al[4 * q + 3] == mhp)) { cnt[UPREF_REJ_MH]++; continue; }
                    if (!((ndp[0] * ndq[0] + ndp[1] * ndq[1]) + ndp[2] * ndq[2] >= 0.0f)) { cnt[UPREF_REJ_NORMAL]++; continue; }
                    const float* L = low + 4 * lq;
                    S[0] = S[0] + g * L[0];
                    S[1] = S[1] + g * L[1];
                    S[2] = S[2] + g * L[2];
                    W = W + g;
                    G2 = G2 + g * g;
                    if (low_vmean) SV = SV + (g * g) * low_vmean[lq];
                    cnt[UPREF_TAKEN]++;
                    ++taken;
                }
                if (!(W >= w_min)) { cnt[UPREF_HOLE_W]++; continue; }
                o[0] = S[0] / W;
                o[1] = S[1] / W;
                o[2] = S[2] / W;
                o[3] = 1.0f;
                if (weight_out) weight_out[p] = (W * W) / G2;
                if (var_out) var_out[p] = SV / (W * W);
                if (!lattice) cnt[UPREF_FROM_1 + taken - 1]++;
            }
    }
    return 0;
}

/* mm_fill_pixels.  image: w*h float4, var and weight: w*h floats or NULL, the window (x0, y0, w, h); pixels: n pairs
 * (x, y); extra: n float4; extra_vmean: n floats (with var).  Returns the number of entries inside the window. */
uint64_t upref_fill(float* image, float* var, float* weight, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                    const uint32_t* pixels, const float* extra, const float* extra_vmean, uint64_t n, float m) {
    uint64_t inside = 0;
    for (uint64_t e = 0; e < n; ++e) {
        const uint32_t x = pixels[2 * e], y = pixels[2 * e + 1];
        if (x < x0 || x - x0 >= w || y < y0 || y - y0 >= h) continue;
        const size_t p = (size_t)(y - y0) * w + (x - x0);
        for (int c = 0; c < 4; ++c) image[4 * p + c] = extra[4 * e + c];
        if (var) var[p] = extra_vmean[e];
        if (weight) weight[p] = m;
        ++inside;
    }
    return inside;
}
