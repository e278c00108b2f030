/* temporal_ref.c -- TEST INFRASTRUCTURE: a plain C statement of the temporal
 * accumulation mm_accumulate_frames computes (include/mm_api.h), IEEE binary32
 * in the order written there, built with the oracle Makefile's CFLAGS
 * (-ffp-contract=off, no fast-math).  tests/temporal_support.py binds it.
 *
 * Besides the accumulated frames it counts what every pixel and every history
 * tap of a call met: TPREF_N_COUNTS uint64 (see the enum), so that a test can
 * tell whether its inputs made every clause decide something. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../include/mm_types.h"

enum {
    TPREF_NO_FRAME = 0,  /* pixels: there is no history frame                          */
    TPREF_MISS,          /* pixels: id is MM_AOV_ID_MISS or MM_AOV_ID_FAILED            */
    TPREF_BEHIND,        /* pixels: not l.z > 0 (the point is behind the history camera) */
    TPREF_OUT_OF_WINDOW, /* pixels: the projection falls outside [-1, w) x [-1, h)      */
    TPREF_TAP_OUTSIDE,   /* taps skipped: q outside the tile                            */
    TPREF_REJ_ID,        /* taps skipped: id'_q != id_p                                 */
    TPREF_REJ_MH,        /* ... ids equal, al'_q.w != al_p.w                            */
    TPREF_REJ_NORMAL,    /* ... ids and mirror hits equal, normals' dot < 0             */
    TPREF_REJ_DIST,      /* ... those three hold, the distances differ by more than tol_z */
    TPREF_W_BELOW,       /* pixels: the valid taps' weight is below w_min               */
    TPREF_BLENDED,       /* pixels blended with their history                           */
    TPREF_N_CAPPED,      /* blended pixels whose SN / W + 1 exceeded n_max              */
    TPREF_N_COUNTS
};

typedef struct { float x, y, z; } v3;

static v3 mk(float x, float y, float z) { v3 r = {x, y, z}; return r; }
static float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

/* rot(q, qw, v) of the header */
static v3 rot(v3 q, float qw, v3 v) {
    const v3 nq = mk(-q.x, -q.y, -q.z);
    const float s1 = -dot3(nq, v);
    const v3 c1 = mk(nq.y * v.z - nq.z * v.y, nq.z * v.x - nq.x * v.z, nq.x * v.y - nq.y * v.x);
    const v3 v1 = mk(c1.x + qw * v.x, c1.y + qw * v.y, c1.z + qw * v.z);
    const v3 c2 = mk(v1.y * q.z - v1.z * q.y, v1.z * q.x - v1.x * q.z, v1.x * q.y - v1.y * q.x);
    return mk((qw * v1.x + s1 * q.x) + c2.x, (qw * v1.y + s1 * q.y) + c2.y, (qw * v1.z + s1 * q.z) + c2.z);
}

/* The primary direction of pixel (px, py): oracle/mm_oracle.c's primary_dir, which mm_trace_aov's kernel runs. */
static v3 primary_dir(const mm_camera* c, float view_w, float view_h, uint32_t px, uint32_t py) {
    const float fx = (float)px, fy = (float)py;
    const v3 p = mk((c->viewport[0] * fx) / view_w - c->viewport[0] * 0.5f,
                    (c->viewport[1] * fy) / view_h - c->viewport[1] * 0.5f, 0.0f - (-c->focal));
    const float s = 1.0f / sqrtf(dot3(p, p));
    return rot(mk(c->quat[0], c->quat[1], c->quat[2]), c->quat[3], mk(s * p.x, s * p.y, s * p.z));
}

typedef struct {
    const float *color, *nd, *al;
    const uint32_t* id;
    const mm_camera* cam;
} frame_t;

/* One frame: cur (traced), hist (NULL: none; its color is an output of this function), out. */
static void one_frame(const frame_t* cur, const frame_t* hist, float view_w, float view_h, uint32_t x0, uint32_t y0,
                      uint32_t w, uint32_t h, float n_max, float tol_z, float w_min, float* out, uint64_t* cnt) {
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const size_t p = (size_t)j * w + i;
            const float* C = cur->color + 4 * p;
            float* o = out + 4 * p;
            o[0] = C[0]; o[1] = C[1]; o[2] = C[2]; o[3] = 1.0f;  /* NOHIST, until the history is found valid */
            if (!hist) { cnt[TPREF_NO_FRAME]++; continue; }
            const uint32_t idp = cur->id[p];
            if (idp == MM_AOV_ID_MISS || idp == MM_AOV_ID_FAILED) { cnt[TPREF_MISS]++; continue; }
            const float* ndp = cur->nd + 4 * p;
            const float mhp = cur->al[4 * p + 3];
            const mm_camera* cam = cur->cam;
            const mm_camera* hc = hist->cam;
            const v3 d = primary_dir(cam, view_w, view_h, x0 + i, y0 + j);
            const v3 X = mk(cam->center[0] + ndp[3] * d.x, cam->center[1] + ndp[3] * d.y, cam->center[2] + ndp[3] * d.z);
            const v3 r = mk(X.x - hc->center[0], X.y - hc->center[1], X.z - hc->center[2]);
            const v3 l = rot(mk(-hc->quat[0], -hc->quat[1], -hc->quat[2]), hc->quat[3], r);
            const float dp = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);
            if (!(l.z > 0.0f)) { cnt[TPREF_BEHIND]++; continue; }
            const float sx = ((((l.x * hc->focal) / l.z) + hc->viewport[0] * 0.5f) * view_w) / hc->viewport[0];
            const float sy = ((((l.y * hc->focal) / l.z) + hc->viewport[1] * 0.5f) * view_h) / hc->viewport[1];
            const float u = sx - (float)x0, v = sy - (float)y0;
            if (!(u >= -1.0f && u < (float)w && v >= -1.0f && v < (float)h)) { cnt[TPREF_OUT_OF_WINDOW]++; continue; }
            const float fu = floorf(u), fv = floorf(v);
            const float a = u - fu, b = v - fv;
            const int i0 = (int)fu, j0 = (int)fv;
            float S[3] = {0.0f, 0.0f, 0.0f}, SN = 0.0f, W = 0.0f;
            for (int t = 0; t < 4; ++t) {
                const int dx = t & 1, dy = t >> 1;
                const int64_t qx = (int64_t)i0 + dx, qy = (int64_t)j0 + dy;
                if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) { cnt[TPREF_TAP_OUTSIDE]++; continue; }
                const size_t q = (size_t)qy * w + (size_t)qx;
                const float* ndq = hist->nd + 4 * q;
                const float* Hq = hist->color + 4 * q;
                if (hist->id[q] != idp) { cnt[TPREF_REJ_ID]++; continue; }
                if (!(hist->al[4 * q + 3] == mhp)) { cnt[TPREF_REJ_MH]++; continue; }
                if (!((ndp[0] * ndq[0] + ndp[1] * ndq[1]) + ndp[2] * ndq[2] >= 0.0f)) { cnt[TPREF_REJ_NORMAL]++; continue; }
                if (!(fabsf(dp - ndq[3]) <= tol_z * (dp + ndq[3]))) { cnt[TPREF_REJ_DIST]++; continue; }
                const float g = (dx ? a : 1.0f - a) * (dy ? b : 1.0f - b);
                S[0] = S[0] + g * Hq[0];
                S[1] = S[1] + g * Hq[1];
                S[2] = S[2] + g * Hq[2];
                SN = SN + g * Hq[3];
                W = W + g;
            }
            if (!(W >= w_min)) { cnt[TPREF_W_BELOW]++; continue; }
            const float t = SN / W + 1.0f;
            const float N = fminf(t, n_max);
            for (int c = 0; c < 3; ++c) {
                const float Hc = S[c] / W;
                o[c] = Hc + (C[c] - Hc) / N;
            }
            o[3] = N;
            cnt[TPREF_BLENDED]++;
            if (t > n_max) cnt[TPREF_N_CAPPED]++;
        }
}

/* cams: n_frames mm_camera; color, nd, al: n_frames*w*h float4; id: n_frames*w*h; the p_* arguments: the prev
 * frame (p_color NULL: none); out: n_frames*w*h float4, not overlapping an input; counts: TPREF_N_COUNTS uint64,
 * added to (NULL: not kept).  Returns 0, or -1 for arguments mm_accumulate_frames rejects. */
int tpref_accumulate(float view_w, float view_h, const mm_camera* cams, const float* color, const float* nd,
                     const float* al, const uint32_t* id, const float* p_color, const float* p_nd, const float* p_al,
                     const uint32_t* p_id, const mm_camera* p_cam, uint32_t n_max, float tol_z, float w_min,
                     uint32_t n_frames, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float* out, uint64_t* counts) {
    uint64_t local[TPREF_N_COUNTS] = {0};
    if (!cams || !color || !nd || !al || !id || !out || !w || !h || !n_frames) return -1;
    if (p_color && (!p_nd || !p_al || !p_id || !p_cam)) return -1;
    if (n_max < 1 || n_max > 65535 || !(tol_z > 0.0f) || !isfinite(tol_z) || !(w_min > 0.0f && w_min <= 1.0f)) return -1;
    if ((uint64_t)x0 + w > (1u << 24) || (uint64_t)y0 + h > (1u << 24)) return -1;
    const size_t n = (size_t)w * h;
    frame_t hist = {p_color, p_nd, p_al, p_id, p_cam};
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * n;
        const frame_t cur = {color + 4 * o, nd + 4 * o, al + 4 * o, id + o, cams + f};
        one_frame(&cur, hist.color ? &hist : NULL, view_w, view_h, x0, y0, w, h, (float)n_max, tol_z, w_min,
                  out + 4 * o, counts ? counts : local);
        hist = cur;
        hist.color = out + 4 * o;
    }
    return 0;
}

int tpref_n_counts(void) { return TPREF_N_COUNTS; }
