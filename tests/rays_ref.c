/* rays_ref.c -- TEST INFRASTRUCTURE: the expected output of mm_trace_rays
 * (include/mm_api.h), IEEE binary32 in the order written there, built with the
 * oracle Makefile's CFLAGS (-ffp-contract=off, no fast-math).
 * tests/rays_support.py binds it.
 *
 * What is stated here is the resolve -- an entry's mean in the order T and its
 * variance, from the entry's spp sample values -- and, for MM_RAYS_JITTER, the
 * two draws and the addition.  The samples themselves are the oracle's:
 * oracle/mm_oracle.c is included (as tests/variance_ref.c does), and sample s of
 * an entry is its trace_path from the record's origin and direction with the
 * seed oracle_tile_seed(key, s, frame). */
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

/* out[4] = (T(s.r), T(s.g), T(s.b)) / (float)spp, alpha 1; *var (spp >= 2, else 0) as mm_api.h defines it.
 * x: spp floats of scratch */
static void resolve_entry(const v3* s, uint32_t spp, float* x, float out[4], float* var) {
    const float m = (float)spp;
    for (uint32_t k = 0; k < spp; ++k) x[k] = s[k].x;
    out[0] = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = s[k].y;
    out[1] = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = s[k].z;
    out[2] = sum_T(x, spp) / m;
    out[3] = 1.0f;
    *var = 0.0f;
    if (spp < 2) return;
    for (uint32_t k = 0; k < spp; ++k) x[k] = lum3(s[k]);
    const float ml = sum_T(x, spp) / m;
    for (uint32_t k = 0; k < spp; ++k) x[k] = (lum3(s[k]) - ml) * (lum3(s[k]) - ml);
    *var = sum_T(x, spp) / (float)(spp - 1u);
}

/* MM_RAYS_JITTER: dir = d + (j1*0.001f, j2*0.001f, 0.0f*0.001f), j1 and j2 the seed's first two draws */
static v3 ray_jitter(v3 d, uint32_t* seed) {
    const float j1 = oracle_rand_pm1(seed);
    const float j2 = oracle_rand_pm1(seed);
    return mk(d.x + j1 * 0.001f, d.y + j2 * 0.001f, d.z + 0.0f * 0.001f);
}

/* The direction sample `smp` of a record starts with (for the test of the restatement itself). */
void raysref_dir(const float rec[8], uint32_t smp, uint32_t frame, int jitter, float dir[3]) {
    uint32_t key;
    memcpy(&key, &rec[3], 4);
    uint32_t seed = oracle_tile_seed(key, smp, frame);
    const unsigned saved = fp_enter();
    v3 d = mk(rec[4], rec[5], rec[6]);
    if (jitter) d = ray_jitter(d, &seed);
    fp_leave(saved);
    dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
}

/* rays: n records of 8 words (ox, oy, oz, key bits, dx, dy, dz, -); out: n x 4; var: n; *n_queries: the
 * closest-hit queries of all paths (mm_stats.rays) */
int raysref_trace(const oracle_scene* sc, const mm_ext* e, int jitter, const float* rays, uint64_t n, float* out,
                  float* var, uint64_t* n_queries) {
    if (!e || e->spp == 0 || e->spp > 4096) return MM_ERR_INVALID;
    v3* s = (v3*)malloc(sizeof(v3) * e->spp);
    float* x = (float*)malloc(sizeof(float) * e->spp);
    int rc = (s && x) ? MM_OK : MM_ERR_NOMEM;
    uint64_t queries = 0;
    trav_t tr = {0, 0, 0};
    const unsigned saved = fp_enter();
    for (uint64_t p = 0; p < n && rc == MM_OK; ++p) {
        const float* r = rays + 8 * p;
        uint32_t key;
        memcpy(&key, &r[3], 4);
        for (uint32_t k = 0; k < e->spp && rc == MM_OK; ++k) {
            uint32_t seed = oracle_tile_seed(key, k, e->frame);
            v3 d = mk(r[4], r[5], r[6]);
            if (jitter) d = ray_jitter(d, &seed);
            s[k] = trace_path(sc, mk(r[0], r[1], r[2]), d, seed, (int)e->bounce_limit, (int)e->mirror_limit, &queries,
                              &tr);
            if (tr.overflow) rc = MM_ERR_STACK;
        }
        if (rc == MM_OK) resolve_entry(s, e->spp, x, out + 4 * p, var + p);
    }
    fp_leave(saved);
    free(s);
    free(x);
    if (n_queries) *n_queries = queries;
    return rc;
}

/* The resolve alone: samples n x spp x 3 floats -> out n x 4, var n */
int raysref_resolve(const float* samples, uint64_t n, uint32_t spp, float* out, float* var) {
    if (spp == 0 || spp > 4096) return MM_ERR_INVALID;
    float* x = (float*)malloc(sizeof(float) * spp);
    if (!x) return MM_ERR_NOMEM;
    const unsigned saved = fp_enter();
    for (uint64_t p = 0; p < n; ++p)
        resolve_entry((const v3*)(samples + 3 * (size_t)p * spp), spp, x, out + 4 * p, var + p);
    fp_leave(saved);
    free(x);
    return MM_OK;
}
