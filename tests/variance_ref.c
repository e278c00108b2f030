/* variance_ref.c -- TEST INFRASTRUCTURE: a plain C statement of the per-pixel
 * sample variance of mm_trace_tile_var / mm_trace_pixels_var (include/mm_api.h),
 * IEEE binary32 in the order written there, built with the oracle Makefile's
 * CFLAGS (-ffp-contract=off, no fast-math).  tests/variance_support.py binds it.
 *
 * Two entry points: varref_samples takes the samples themselves; varref_tile /
 * varref_pixels trace them with the oracle's own functions (oracle/mm_oracle.c
 * is included, as tests/aov_ref.c does), restating oracle_trace_tile_body's
 * sample loop so that the samples -- and the mean -- are the oracle's.
 *
 * With -DVARREF_MAIN it is a stand-alone program (for a sanitizer build): it
 * takes the variance of seeded samples at every spp the tests use, traces a
 * small hand-built room as a tile and as a pixel list, and prints a checksum
 * of all the results' bits. */
#include "../oracle/mm_oracle.c"

static float lum3(v3 s) { return (0.25f * s.x + 0.5f * s.y) + 0.25f * s.z; }

/* T(x): the resolve's summation order over x[0 .. spp-1] */
static float sum_T(const float* x, uint32_t spp) {
    float acc;
    if (spp % 8 == 0) {
        acc = 0.0f;
        for (uint32_t b = 0; b < spp; b += 8) {
            const float p0 = x[b + 0] + x[b + 1], p1 = x[b + 2] + x[b + 3];
            const float p2 = x[b + 4] + x[b + 5], p3 = x[b + 6] + x[b + 7];
            const float blk = (p0 + p1) + (p2 + p3);
            acc = (b == 0) ? blk : acc + blk;
        }
    } else {
        acc = x[0];
        for (uint32_t k = 1; k < spp; ++k) acc = acc + x[k];
    }
    return acc;
}

/* mean[3] and var of one pixel's samples s[0 .. spp-1] (spp >= 2); x: spp floats of scratch */
static void pixel_moments(const v3* s, uint32_t spp, float* x, float mean[3], float* var) {
    const float m = (float)spp;
    for (uint32_t k = 0; k < spp; ++k) x[k] = s[k].x;
    mean[0] = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = s[k].y;
    mean[1] = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = s[k].z;
    mean[2] = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = lum3(s[k]);
    const float ml = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = (lum3(s[k]) - ml) * (lum3(s[k]) - ml);
    *var = sum_T(x, spp) / (float)(spp - 1u);
}

/* samples: n_pix x spp x 3 floats; mean: n_pix x 3; var: n_pix */
int varref_samples(const float* samples, uint64_t n_pix, uint32_t spp, float* mean, float* var) {
    if (spp < 2 || spp > 4096) return MM_ERR_INVALID;
    float* x = (float*)malloc(sizeof(float) * spp);
    if (!x) return MM_ERR_NOMEM;
    const unsigned saved = fp_enter();
    for (uint64_t p = 0; p < n_pix; ++p)
        pixel_moments((const v3*)(samples + 3 * (size_t)p * spp), spp, x, mean + 3 * p, var + p);
    fp_leave(saved);
    free(x);
    return MM_OK;
}

/* The samples of view pixel (px, py), as oracle_trace_tile_body draws and traces them. */
static int pixel_samples(const oracle_scene* sc, const mm_uniform* u, const mm_ext* e, uint32_t px, uint32_t py,
                         v3* s) {
    const uint32_t pixel = py * (uint32_t)u->view_w + px;
    const v3 d0 = primary_dir(u, px, py);
    uint64_t rays = 0;
    trav_t tr = {0, 0, 0};
    for (uint32_t k = 0; k < e->spp; ++k) {
        uint32_t seed = oracle_tile_seed(pixel, k, e->frame);
        v3 d = jittered_dir(d0, &seed);
        s[k] = trace_path(sc, ld3(u->cam.center), d, seed, (int)e->bounce_limit, (int)e->mirror_limit, &rays, &tr);
        if (tr.overflow) return MM_ERR_STACK;
    }
    return MM_OK;
}

/* pixels: NULL (the tile (x0 + i, y0 + j * y_stride), n = w * h) or n pairs (x, y); out: n x 4, var: n */
static int trace_var(const oracle_scene* sc, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels, uint64_t n,
                     uint32_t x0, uint32_t y0, uint32_t w, uint32_t y_stride, float* out, float* var) {
    if (!e || e->spp < 2 || e->spp > 4096) return MM_ERR_INVALID;
    v3* s = (v3*)malloc(sizeof(v3) * e->spp);
    float* x = (float*)malloc(sizeof(float) * e->spp);
    int rc = (s && x) ? MM_OK : MM_ERR_NOMEM;
    const unsigned saved = fp_enter();
    for (uint64_t p = 0; p < n && rc == MM_OK; ++p) {
        const uint32_t px = pixels ? pixels[2 * p] : x0 + (uint32_t)(p % w);
        const uint32_t py = pixels ? pixels[2 * p + 1] : y0 + (uint32_t)(p / w) * y_stride;
        float* o = out + 4 * p;
        if (pixels && !(px < (uint32_t)u->view_w && py < (uint32_t)u->view_h)) {
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            var[p] = 0.0f;
            continue;
        }
        rc = pixel_samples(sc, u, e, px, py, s);
        if (rc) break;
        pixel_moments(s, e->spp, x, o, var + p);
        o[3] = 1.0f;
    }
    fp_leave(saved);
    free(s);
    free(x);
    return rc;
}

int varref_tile(const oracle_scene* sc, const mm_uniform* u, const mm_ext* e, uint32_t x0, uint32_t y0, uint32_t w,
                uint32_t h, uint32_t y_stride, float* out, float* var) {
    if (w == 0 || y_stride == 0) return MM_ERR_INVALID;
    return trace_var(sc, u, e, NULL, (uint64_t)w * h, x0, y0, w, y_stride, out, var);
}

int varref_pixels(const oracle_scene* sc, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels, uint64_t n,
                  float* out, float* var) {
    return trace_var(sc, u, e, pixels, n, 0, 0, 1, 1, out, var);
}

#ifdef VARREF_MAIN
#include <stdio.h>

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

static uint32_t fold(uint32_t sum, const float* v, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t b;
        memcpy(&b, &v[i], 4);
        sum = sum * 31u + b;
    }
    return sum;
}

int main(void) {
    static const uint32_t spps[] = {2, 3, 4, 8, 12, 16, 24, 64};
    enum { NPIX = 37, W = 9, H = 5, NLIST = 12 };
    uint32_t seed = 12345u, sum = 0;
    /* seeded samples in [0, 4) */
    for (size_t i = 0; i < sizeof(spps) / sizeof(spps[0]); ++i) {
        const uint32_t spp = spps[i];
        float* s = malloc(sizeof(float) * 3 * NPIX * spp);
        float* mean = malloc(sizeof(float) * 3 * NPIX);
        float* var = malloc(sizeof(float) * NPIX);
        if (!s || !mean || !var) return 2;
        for (size_t k = 0; k < (size_t)3 * NPIX * spp; ++k) s[k] = (float)(lcg(&seed) >> 8) * 0x1p-22f;
        if (varref_samples(s, NPIX, spp, mean, var)) return 3;
        for (int p = 0; p < NPIX; ++p)
            if (!(var[p] > 0.0f)) return 4;
        sum = fold(fold(sum, mean, 3 * NPIX), var, NPIX);
        free(s); free(mean); free(var);
    }
    /* a closed room, 4 x 4 x 8, one leaf: an emitting ceiling, a mirror at the far end, matte elsewhere */
    static const mm_rect rects[6] = {
        {{-2, -2, 0}, {4, 0, 0}, {0, 0, 8}, {0.8f, 0.8f, 0.8f}},  /* ceiling y = -2 */
        {{-2, 2, 0}, {0, 0, 8}, {4, 0, 0}, {0.6f, 0.5f, 0.4f}},   /* floor y = 2 */
        {{-2, -2, 0}, {0, 0, 8}, {0, 4, 0}, {0.7f, 0.2f, 0.2f}},  /* x = -2 */
        {{2, -2, 0}, {0, 4, 0}, {0, 0, 8}, {0.2f, 0.7f, 0.2f}},   /* x = 2 */
        {{-2, -2, 8}, {0, 4, 0}, {4, 0, 0}, {0.9f, 0.9f, 0.95f}}, /* far end z = 8: the mirror */
        {{-2, -2, 0}, {4, 0, 0}, {0, 4, 0}, {0.5f, 0.5f, 0.5f}},  /* near end z = 0 */
    };
    static const mm_node nodes[1] = {{{-2, -2, 0}, {2, 2, 8}, 0, 6}};
    static const uint32_t idx[6] = {0, 1, 2, 3, 4, 5};
    static const uint8_t is_mirror[6] = {0, 0, 0, 0, 1, 0};
    static const float emission[24] = {1, 1, 0.9f, 2, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0};
    const oracle_scene sc = {rects, 6, nodes, 1, idx, is_mirror, emission};
    mm_uniform u;
    memset(&u, 0, sizeof(u));
    u.cam.center[2] = 1.0f;
    u.cam.focal = 1.0f;
    u.cam.quat[3] = 1.0f;
    u.cam.viewport[0] = 2.0f * 16 / 12;
    u.cam.viewport[1] = 2.0f;
    u.view_w = 16.0f;
    u.view_h = 12.0f;
    u.chunk_w = 4;
    float out[4 * W * H], var[W * H], lout[4 * NLIST], lvar[NLIST];
    uint32_t list[2 * NLIST];
    for (int e = 0; e < NLIST; ++e) {
        list[2 * e] = 3 + lcg(&seed) % W;
        list[2 * e + 1] = 2 + 2 * (lcg(&seed) % H);
    }
    list[0] = 0x80000000u; list[1] = 0x80000000u;  /* outside the view */
    list[2] = 16; list[3] = 0;
    int lit = 0;
    for (size_t i = 0; i < sizeof(spps) / sizeof(spps[0]); ++i) {
        mm_ext e;
        memset(&e, 0, sizeof(e));
        e.spp = spps[i]; e.bounce_limit = 4; e.mirror_limit = 4; e.frame = 7;
        if (varref_tile(&sc, &u, &e, 3, 2, W, H, 2, out, var)) return 5;
        if (varref_pixels(&sc, &u, &e, list, NLIST, lout, lvar)) return 6;
        if (lvar[0] != 0.0f || lvar[1] != 0.0f || lout[3] != 0.0f) return 7;
        for (int k = 2; k < NLIST; ++k) {  /* a list entry is its pixel of the tile */
            const int p = (int)((list[2 * k + 1] - 2) / 2) * W + (int)(list[2 * k] - 3);
            if (memcmp(lout + 4 * k, out + 4 * p, 16) || memcmp(lvar + k, var + p, 4)) return 8;
        }
        for (int p = 0; p < W * H; ++p) lit += var[p] > 0.0f;
        sum = fold(fold(fold(sum, out, 4 * W * H), var, W * H), lvar, NLIST);
    }
    printf("lit %d checksum %08x\n", lit, sum);
    return lit > 0 ? 0 : 1;
}
#endif
