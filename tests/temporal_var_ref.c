/* temporal_var_ref.c -- TEST INFRASTRUCTURE: a plain C statement of what
 * mm_accumulate_frames_var and mm_blend_pixels_var compute (include/mm_api.h),
 * IEEE binary32 in the order written there, built with the oracle Makefile's
 * CFLAGS (-ffp-contract=off, no fast-math).  tests/temporal_var_support.py
 * binds it.
 *
 * Like temporal_ref.c it counts what every pixel and every history tap of a
 * call met: TVREF_N_COUNTS uint64 (see the enum; the first twelve are
 * temporal_ref.c's, in its order), so that a test can tell whether its inputs
 * made every clause decide something. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../include/mm_types.h"

enum {
    TVREF_NO_FRAME = 0,  /* pixels: there is no history frame                          */
    TVREF_MISS,          /* pixels: id is MM_AOV_ID_MISS or MM_AOV_ID_FAILED            */
    TVREF_BEHIND,        /* pixels: not l.z > 0 (the point is behind the history camera) */
    TVREF_OUT_OF_WINDOW, /* pixels: the projection falls outside [-1, w) x [-1, h)      */
    TVREF_TAP_OUTSIDE,   /* taps skipped: q outside the tile                            */
    TVREF_REJ_ID,        /* taps skipped: id'_q != id_p                                 */
    TVREF_REJ_MH,        /* ... ids equal, al'_q.w != al_p.w                            */
    TVREF_REJ_NORMAL,    /* ... ids and mirror hits equal, normals' dot < 0             */
    TVREF_REJ_DIST,      /* ... those three hold, the distances differ by more than tol_z */
    TVREF_W_BELOW,       /* pixels: the valid taps' weight is below w_min               */
    TVREF_BLENDED,       /* pixels blended with their history                           */
    TVREF_N_CAPPED,      /* blended pixels whose SN / W + m exceeded fmaxf(n_max, m)    */
    TVREF_M_ABOVE_CAP,   /* blended pixels whose weight m exceeded n_max (fmaxf picked m) */
    TVREF_TINY_PRODUCT,  /* products (g*g)*V'_q of taken taps and (b*b)*Vc of blended pixels that are subnormal */
    TVREF_N_COUNTS
};

typedef struct { float x, y, z; } v3;

static v3 mk(float x, float y, float z) { v3 r = {x, y, z}; return r; }
static float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static int tiny(float x) { return x != 0.0f && fabsf(x) < FLT_MIN; }

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
    const float* var;    /* cur: vmean; hist: that frame's variance output */
    const float* weight; /* cur only; NULL: 1 everywhere */
} frame_t;

/* One frame: cur (traced), hist (NULL: none; its color and var are outputs of this function), out, vout. */
static void one_frame(const frame_t* cur, const frame_t* hist, float view_w, float view_h, uint32_t x0, uint32_t y0,
                      uint32_t w, uint32_t h, float n_max, float tol_z, float w_min, float* out, float* vout,
                      uint64_t* cnt) {
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const size_t p = (size_t)j * w + i;
            const float* C = cur->color + 4 * p;
            const float m = cur->weight ? cur->weight[p] : 1.0f;
            const float Vc = cur->var[p];
            float* o = out + 4 * p;
            o[0] = C[0]; o[1] = C[1]; o[2] = C[2]; o[3] = m;  /* NOHIST, until the history is found valid */
            vout[p] = Vc;
            if (!hist) { cnt[TVREF_NO_FRAME]++; continue; }
            const uint32_t idp = cur->id[p];
            if (idp == MM_AOV_ID_MISS || idp == MM_AOV_ID_FAILED) { cnt[TVREF_MISS]++; continue; }
            const float* ndp = cur->nd + 4 * p;
            const float mhp = cur->al[4 * p + 3];
            const mm_camera* cam = cur->cam;
            const mm_camera* hc = hist->cam;
            const v3 d = primary_dir(cam, view_w, view_h, x0 + i, y0 + j);
            const v3 X = mk(cam->center[0] + ndp[3] * d.x, cam->center[1] + ndp[3] * d.y, cam->center[2] + ndp[3] * d.z);
            const v3 r = mk(X.x - hc->center[0], X.y - hc->center[1], X.z - hc->center[2]);
            const v3 l = rot(mk(-hc->quat[0], -hc->quat[1], -hc->quat[2]), hc->quat[3], r);
            const float dp = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);
            if (!(l.z > 0.0f)) { cnt[TVREF_BEHIND]++; continue; }
            const float sx = ((((l.x * hc->focal) / l.z) + hc->viewport[0] * 0.5f) * view_w) / hc->viewport[0];
            const float sy = ((((l.y * hc->focal) / l.z) + hc->viewport[1] * 0.5f) * view_h) / hc->viewport[1];
            const float u = sx - (float)x0, v = sy - (float)y0;
            if (!(u >= -1.0f && u < (float)w && v >= -1.0f && v < (float)h)) { cnt[TVREF_OUT_OF_WINDOW]++; continue; }
            const float fu = floorf(u), fv = floorf(v);
            const float a = u - fu, b = v - fv;
            const int i0 = (int)fu, j0 = (int)fv;
            float S[3] = {0.0f, 0.0f, 0.0f}, SN = 0.0f, SV = 0.0f, W = 0.0f;
            uint64_t tiny_taps = 0;
            for (int t = 0; t < 4; ++t) {
                const int dx = t & 1, dy = t >> 1;
                const int64_t qx = (int64_t)i0 + dx, qy = (int64_t)j0 + dy;
                if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) { cnt[TVREF_TAP_OUTSIDE]++; continue; }
                const size_t q = (size_t)qy * w + (size_t)qx;
                const float* ndq = hist->nd + 4 * q;
                const float* Hq = hist->color + 4 * q;
                if (hist->id[q] != idp) { cnt[TVREF_REJ_ID]++; continue; }
                if (!(hist->al[4 * q + 3] == mhp)) { cnt[TVREF_REJ_MH]++; continue; }
                if (!((ndp[0] * ndq[0] + ndp[1] * ndq[1]) + ndp[2] * ndq[2] >= 0.0f)) { cnt[TVREF_REJ_NORMAL]++; continue; }
                if (!(fabsf(dp - ndq[3]) <= tol_z * (dp + ndq[3]))) { cnt[TVREF_REJ_DIST]++; continue; }
                const float g = (dx ? a : 1.0f - a) * (dy ? b : 1.0f - b);
                const float gv = (g * g) * hist->var[q];
                S[0] = S[0] + g * Hq[0];
                S[1] = S[1] + g * Hq[1];
                S[2] = S[2] + g * Hq[2];
                SN = SN + g * Hq[3];
                SV = SV + gv;
                W = W + g;
                if (tiny(gv)) tiny_taps++;
            }
            if (!(W >= w_min)) { cnt[TVREF_W_BELOW]++; continue; }
            const float VH = SV / (W * W);
            const float t = SN / W + m;
            const float cap = fmaxf(n_max, m);
            const float N = fminf(t, cap);
            for (int c = 0; c < 3; ++c) {
                const float Hc = S[c] / W;
                o[c] = Hc + ((C[c] - Hc) * m) / N;
            }
            o[3] = N;
            const float bw = m / N, cw = 1.0f - bw;
            const float bv = (bw * bw) * Vc;
            vout[p] = (cw * cw) * VH + bv;
            cnt[TVREF_BLENDED]++;
            if (t > cap) cnt[TVREF_N_CAPPED]++;
            if (m > n_max) cnt[TVREF_M_ABOVE_CAP]++;
            cnt[TVREF_TINY_PRODUCT] += tiny_taps + (tiny(bv) ? 1 : 0);
        }
}

/* cams: n_frames mm_camera; color, nd, al: n_frames*w*h float4; id, vmean: n_frames*w*h; weight: n_frames*w*h or
 * NULL; the p_* arguments: the prev frame (p_color NULL: none); out: n_frames*w*h float4, var_out: n_frames*w*h,
 * neither overlapping an input; counts: TVREF_N_COUNTS uint64, added to (NULL: not kept).  Returns 0, or -1 for
 * arguments mm_accumulate_frames_var rejects. */
int tvref_accumulate(float view_w, float view_h, const mm_camera* cams, const float* color, const float* nd,
                     const float* al, const uint32_t* id, const float* vmean, const float* weight,
                     const float* p_color, const float* p_nd, const float* p_al, const uint32_t* p_id,
                     const mm_camera* p_cam, const float* p_var, uint32_t n_max, float tol_z, float w_min,
                     uint32_t n_frames, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float* out, float* var_out,
                     uint64_t* counts) {
    uint64_t local[TVREF_N_COUNTS] = {0};
    if (!cams || !color || !nd || !al || !id || !vmean || !out || !var_out || !w || !h || !n_frames) return -1;
    if (p_color && (!p_nd || !p_al || !p_id || !p_cam || !p_var)) return -1;
    if (n_max < 1 || n_max > 65535 || !(tol_z > 0.0f) || !isfinite(tol_z) || !(w_min > 0.0f && w_min <= 1.0f)) return -1;
    if ((uint64_t)x0 + w > (1u << 24) || (uint64_t)y0 + h > (1u << 24)) return -1;
    const size_t n = (size_t)w * h;
    frame_t hist = {p_color, p_nd, p_al, p_id, p_cam, p_var, NULL};
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * n;
        const frame_t cur = {color + 4 * o, nd + 4 * o, al + 4 * o, id + o, cams + f, vmean + o,
                             weight ? weight + o : NULL};
        one_frame(&cur, hist.color ? &hist : NULL, view_w, view_h, x0, y0, w, h, (float)n_max, tol_z, w_min,
                  out + 4 * o, var_out + o, counts ? counts : local);
        hist = cur;
        hist.color = out + 4 * o;
        hist.var = var_out + o;
        hist.weight = NULL;
    }
    return 0;
}

int tvref_n_counts(void) { return TVREF_N_COUNTS; }

/* mm_blend_pixels_var.  image: w*h float4 and var: w*h floats, the window (x0, y0, w, h); pixels: n pairs (x, y);
 * extra: n float4; extra_vmean: n floats.  Entries in list order.  Returns the number of entries inside the window. */
uint64_t tvref_blend(float* image, float* var, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                     const uint32_t* pixels, const float* extra, const float* extra_vmean, uint64_t n, float m) {
    uint64_t inside = 0;
    for (uint64_t e = 0; e < n; ++e) {
        const uint32_t x = pixels[2 * e], y = pixels[2 * e + 1];
        if (x < x0 || x - x0 >= w || y < y0 || y - y0 >= h) continue;
        const size_t p = (size_t)(y - y0) * w + (x - x0);
        float* A = image + 4 * p;
        const float* E = extra + 4 * e;
        const float Nn = A[3] + m;
        for (int c = 0; c < 3; ++c) A[c] = A[c] + ((E[c] - A[c]) * m) / Nn;
        A[3] = Nn;
        const float bw = m / Nn, cw = 1.0f - bw;
        var[p] = (cw * cw) * var[p] + (bw * bw) * extra_vmean[e];
        ++inside;
    }
    return inside;
}
