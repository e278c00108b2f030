/* denoise_ref.c -- TEST INFRASTRUCTURE: a plain C statement of the edge-aware
 * a-trous filter mm_denoise_frames computes (include/mm_api.h), IEEE binary32
 * in the order written there, built with the oracle Makefile's CFLAGS
 * (-ffp-contract=off, no fast-math).  tests/denoise_support.py binds it.
 *
 * Besides the filtered image it counts, over all passes of a call, what the
 * taps met: DNREF_N_COUNTS uint64 (see the enum), so that a test can tell
 * whether its inputs made every clause of the filter decide something. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum {
    DNREF_OUT_OF_TILE = 0, /* taps skipped: q outside the tile                    */
    DNREF_REJ_ID,          /* taps skipped: id_q != id_p                          */
    DNREF_REJ_MH,          /* ... ids equal, al_q.w != al_p.w                     */
    DNREF_REJ_NORMAL,      /* ... ids and mirror hits equal, normals' dot < 0     */
    DNREF_SOFT_Z,          /* taken taps whose depth factor 1/(1+t*t) is < 1/2    */
    DNREF_SOFT_L,          /* taken taps whose luminance factor is < 1/2          */
    DNREF_TAKEN,           /* taps taken, the centre included                     */
    DNREF_N_COUNTS
};

static float lum(const float* c) { return (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2]; }

static void one_pass(const float* C, const float* nd, const float* al, const uint32_t* id, uint32_t pass,
                     float sigma_z, float sigma_l, uint32_t w, uint32_t h, float* out, uint64_t* cnt) {
    static const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const int64_t s = (int64_t)1 << pass;
    const float sl = sigma_l * (1.0f / (float)s);
    for (int64_t y = 0; y < (int64_t)h; ++y)
        for (int64_t x = 0; x < (int64_t)w; ++x) {
            const size_t p = (size_t)y * w + (size_t)x;
            const float* Cp = C + 4 * p;
            const float* ndp = nd + 4 * p;
            const float lp = lum(Cp);
            float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int64_t qx = x + s * dx, qy = y + s * dy;
                    if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) {
                        cnt[DNREF_OUT_OF_TILE]++;
                        continue;
                    }
                    const size_t q = (size_t)qy * w + (size_t)qx;
                    const float* Cq = C + 4 * q;
                    const float* ndq = nd + 4 * q;
                    if (!(dx == 0 && dy == 0)) {
                        if (id[q] != id[p]) { cnt[DNREF_REJ_ID]++; continue; }
                        if (!(al[4 * q + 3] == al[4 * p + 3])) { cnt[DNREF_REJ_MH]++; continue; }
                        const float d = (ndp[0] * ndq[0] + ndp[1] * ndq[1]) + ndp[2] * ndq[2];
                        if (!(d >= 0.0f)) { cnt[DNREF_REJ_NORMAL]++; continue; }
                    }
                    float g = hk[dy + 2] * hk[dx + 2];
                    if (sigma_z > 0.0f) {
                        const float t = (ndp[3] - ndq[3]) / (sigma_z * (ndp[3] + ndq[3]));
                        const float f = 1.0f + t * t;
                        if (f > 2.0f) cnt[DNREF_SOFT_Z]++;
                        g = g / f;
                    }
                    if (sigma_l > 0.0f) {
                        const float t = (lp - lum(Cq)) / sl;
                        const float f = 1.0f + t * t;
                        if (f > 2.0f) cnt[DNREF_SOFT_L]++;
                        g = g / f;
                    }
                    S[0] = S[0] + g * Cq[0];
                    S[1] = S[1] + g * Cq[1];
                    S[2] = S[2] + g * Cq[2];
                    W = W + g;
                    cnt[DNREF_TAKEN]++;
                }
            out[4 * p + 0] = S[0] / W;
            out[4 * p + 1] = S[1] / W;
            out[4 * p + 2] = S[2] / W;
            out[4 * p + 3] = Cp[3];
        }
}

/* color, nd, al: n_frames*w*h float4; id: n_frames*w*h; out: n_frames*w*h
 * float4, not overlapping color; counts: DNREF_N_COUNTS uint64, added to (NULL:
 * not kept).  Returns 0, or -1 for arguments mm_denoise_frames rejects. */
int dnref_filter(const float* color, const float* nd, const float* al, const uint32_t* id, uint32_t n_passes,
                 float sigma_z, float sigma_l, uint32_t n_frames, uint32_t w, uint32_t h, float* out,
                 uint64_t* counts) {
    uint64_t local[DNREF_N_COUNTS] = {0};
    if (!color || !nd || !al || !id || !out || n_passes < 1 || n_passes > 8 || !w || !h || !n_frames) return -1;
    const size_t n = (size_t)w * h;
    float* tmp = (float*)malloc(2 * n * 4 * sizeof(float));
    if (!tmp) return -1;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * n;
        const float* src = color + 4 * o;
        for (uint32_t i = 0; i < n_passes; ++i) {
            float* dst = (i + 1 == n_passes) ? out + 4 * o : tmp + (size_t)(i & 1u) * n * 4;
            one_pass(src, nd + 4 * o, al + 4 * o, id + o, i, sigma_z, sigma_l, w, h, dst, counts ? counts : local);
            src = dst;
        }
    }
    free(tmp);
    return 0;
}

int dnref_n_counts(void) { return DNREF_N_COUNTS; }
