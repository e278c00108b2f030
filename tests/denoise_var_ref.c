/* denoise_var_ref.c -- TEST INFRASTRUCTURE: a plain C statement of the
 * variance-guided a-trous filter mm_denoise_frames_var computes
 * (include/mm_api.h), IEEE binary32 with subnormals, in the order written
 * there, built with the oracle Makefile's CFLAGS (-ffp-contract=off, no
 * fast-math).  tests/denoise_var_support.py binds it.
 *
 * Besides the filtered colour and variance it counts, over all passes of a
 * call, what the taps met: DNVREF_N_COUNTS uint64 (see the enum; the first
 * seven are denoise_ref.c's), so that a test can tell whether its inputs made
 * every clause of the filter decide something. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum {
    DNVREF_OUT_OF_TILE = 0, /* taps skipped: q outside the tile                    */
    DNVREF_REJ_ID,          /* taps skipped: id_q != id_p                          */
    DNVREF_REJ_MH,          /* ... ids equal, al_q.w != al_p.w                     */
    DNVREF_REJ_NORMAL,      /* ... ids and mirror hits equal, normals' dot < 0     */
    DNVREF_SOFT_Z,          /* taken taps whose depth factor 1/(1+t*t) is < 1/2    */
    DNVREF_SOFT_L,          /* taken taps whose luminance factor is < 1/2          */
    DNVREF_TAKEN,           /* taps taken, the centre included                     */
    DNVREF_PRE_OUT_OF_TILE, /* the stop's 3x3: taps outside the tile               */
    DNVREF_PRE_REJ_ID,      /* ... rejected by the id                              */
    DNVREF_PRE_REJ_MH,      /* ... by the mirror hits                              */
    DNVREF_PRE_REJ_NORMAL,  /* ... by the normals                                  */
    DNVREF_PRE_TAKEN,       /* ... taken, the centre included                      */
    DNVREF_TINY_PRODUCT,    /* taken taps with V_q > 0 whose (g*g)*V_q is subnormal or zero */
    DNVREF_STOP_IS_EPS,     /* pixels whose stop is eps_l exactly (GV == 0)        */
    DNVREF_N_COUNTS
};

static float lum(const float* c) { return (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2]; }

/* 0: the same surface; else the counter offset (1..3) of the clause that rejects q. */
static int rejected(const float* nd, const float* al, const uint32_t* id, size_t p, size_t q) {
    if (id[q] != id[p]) return 1;
    if (!(al[4 * q + 3] == al[4 * p + 3])) return 2;
    const float* a = nd + 4 * p;
    const float* b = nd + 4 * q;
    const float d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    if (!(d >= 0.0f)) return 3;
    return 0;
}

static void one_pass(const float* C, const float* V, const float* nd, const float* al, const uint32_t* id,
                     uint32_t pass, float sigma_z, float sigma_l, float eps_l, uint32_t w, uint32_t h, float* out,
                     float* vout, uint64_t* cnt) {
    static const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    static const float k3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    const int64_t s = (int64_t)1 << pass;
    for (int64_t y = 0; y < (int64_t)h; ++y)
        for (int64_t x = 0; x < (int64_t)w; ++x) {
            const size_t p = (size_t)y * w + (size_t)x;
            const float* Cp = C + 4 * p;
            const float* ndp = nd + 4 * p;
            const float lp = lum(Cp);
            float slp = 0.0f;
            if (sigma_l > 0.0f) {
                float GV = 0.0f, GW = 0.0f;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int64_t qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) {
                            cnt[DNVREF_PRE_OUT_OF_TILE]++;
                            continue;
                        }
                        const size_t q = (size_t)qy * w + (size_t)qx;
                        if (!(dx == 0 && dy == 0)) {
                            const int r = rejected(nd, al, id, p, q);
                            if (r) { cnt[DNVREF_PRE_REJ_ID + r - 1]++; continue; }
                        }
                        const float g = k3[dy + 1] * k3[dx + 1];
                        GV = GV + g * V[q];
                        GW = GW + g;
                        cnt[DNVREF_PRE_TAKEN]++;
                    }
                slp = sigma_l * sqrtf(GV / GW) + eps_l;
                if (GV == 0.0f) cnt[DNVREF_STOP_IS_EPS]++;
            }
            float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f, SV = 0.0f;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int64_t qx = x + s * dx, qy = y + s * dy;
                    if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) {
                        cnt[DNVREF_OUT_OF_TILE]++;
                        continue;
                    }
                    const size_t q = (size_t)qy * w + (size_t)qx;
                    const float* Cq = C + 4 * q;
                    const float* ndq = nd + 4 * q;
                    if (!(dx == 0 && dy == 0)) {
                        const int r = rejected(nd, al, id, p, q);
                        if (r) { cnt[DNVREF_REJ_ID + r - 1]++; continue; }
                    }
                    float g = hk[dy + 2] * hk[dx + 2];
                    if (sigma_z > 0.0f) {
                        const float t = (ndp[3] - ndq[3]) / (sigma_z * (ndp[3] + ndq[3]));
                        const float f = 1.0f + t * t;
                        if (f > 2.0f) cnt[DNVREF_SOFT_Z]++;
                        g = g / f;
                    }
                    if (sigma_l > 0.0f) {
                        const float t = (lp - lum(Cq)) / slp;
                        const float f = 1.0f + t * t;
                        if (f > 2.0f) cnt[DNVREF_SOFT_L]++;
                        g = g / f;
                    }
                    S[0] = S[0] + g * Cq[0];
                    S[1] = S[1] + g * Cq[1];
                    S[2] = S[2] + g * Cq[2];
                    W = W + g;
                    const float gv = (g * g) * V[q];
                    if (V[q] > 0.0f && gv < 0x1p-126f) cnt[DNVREF_TINY_PRODUCT]++;
                    SV = SV + gv;
                    cnt[DNVREF_TAKEN]++;
                }
            out[4 * p + 0] = S[0] / W;
            out[4 * p + 1] = S[1] / W;
            out[4 * p + 2] = S[2] / W;
            out[4 * p + 3] = Cp[3];
            vout[p] = SV / (W * W);
        }
}

/* color, nd, al: n_frames*w*h float4; id, vmean: n_frames*w*h; out:
 * n_frames*w*h float4 and var_out: n_frames*w*h floats, neither overlapping an
 * input; counts: DNVREF_N_COUNTS uint64, added to (NULL: not kept).  Returns 0,
 * or -1 for arguments mm_denoise_frames_var rejects. */
int dnvref_filter(const float* color, const float* nd, const float* al, const uint32_t* id, const float* vmean,
                  uint32_t n_passes, float sigma_z, float sigma_l, float eps_l, uint32_t n_frames, uint32_t w,
                  uint32_t h, float* out, float* var_out, uint64_t* counts) {
    uint64_t local[DNVREF_N_COUNTS] = {0};
    if (!color || !nd || !al || !id || !vmean || !out || !var_out || n_passes < 1 || n_passes > 8 || !w || !h ||
        !n_frames)
        return -1;
    if (sigma_l > 0.0f && !(eps_l > 0.0f && isfinite(eps_l))) return -1;
    const size_t n = (size_t)w * h;
    float* tmp = (float*)malloc(2 * n * 5 * sizeof(float));
    if (!tmp) return -1;
    float* tmpv = tmp + 2 * n * 4;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * n;
        const float* src = color + 4 * o;
        const float* srcv = vmean + o;
        for (uint32_t i = 0; i < n_passes; ++i) {
            const int last = i + 1 == n_passes;
            float* dst = last ? out + 4 * o : tmp + (size_t)(i & 1u) * n * 4;
            float* dstv = last ? var_out + o : tmpv + (size_t)(i & 1u) * n;
            one_pass(src, srcv, nd + 4 * o, al + 4 * o, id + o, i, sigma_z, sigma_l, eps_l, w, h, dst, dstv,
                     counts ? counts : local);
            src = dst;
            srcv = dstv;
        }
    }
    free(tmp);
    return 0;
}

int dnvref_n_counts(void) { return DNVREF_N_COUNTS; }
