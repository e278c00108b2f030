/*
 * aov_ref.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of mm_query_rays and
 * mm_trace_aov (include/mm_api.h), built from the oracle's own functions the
 * way oracle/grid_cpu.c builds on them.  tests/test_aov.py and
 * tests/test_gpu_aov.py compile it into a temporary directory with the oracle
 * Makefile's CFLAGS.
 */
#include "../oracle/mm_oracle.c"

#define AOV_MISS 0xFFFFFFFFu
#define AOV_FAILED 0xFFFFFFFEu

/* The (t, k) intersect_bvh_iterative ends with when started at t = 1e30
 * (k starts as AOV_MISS, which a miss leaves).  Returns 0, or MM_ERR_STACK
 * with (1e30, AOV_FAILED). */
static int query(const oracle_scene* sc, v3 o, v3 d, float* t, uint32_t* k) {
    ray_t b;
    trav_t tr = {0, 0, 0};
    b.ori = o; b.dir = d; b.t = BIG; b.index = AOV_MISS;
    intersect_bvh(&b, sc, &tr);
    if (tr.overflow) {
        *t = BIG; *k = AOV_FAILED;
        return MM_ERR_STACK;
    }
    *t = b.t;
    *k = b.t < BIG ? b.index : AOV_MISS;
    return MM_OK;
}

int aovref_query(const oracle_scene* sc, const float o[3], const float d[3], float* t, uint32_t* k) {
    const unsigned saved = fp_enter();
    const int rc = query(sc, ld3(o), ld3(d), t, k);
    fp_leave(saved);
    return rc;
}

/* rays: n x (o.xyz, -, d.xyz, -); hits: n x (float t, uint32 k) */
int aovref_query_batch(const oracle_scene* sc, const float* rays, uint64_t n, void* hits) {
    int rc = MM_OK;
    for (uint64_t i = 0; i < n; ++i) {
        float t;
        uint32_t k;
        const int r = aovref_query(sc, rays + 8 * i, rays + 8 * i + 4, &t, &k);
        if (r) rc = r;
        memcpy((char*)hits + 8 * i, &t, 4);
        memcpy((char*)hits + 8 * i + 4, &k, 4);
    }
    return rc;
}

/* The deterministic part of trace_path for the centre ray of pixel (px, py):
 * nd = (side * nn, dist), al = (colour, mirror hits), id = k | kind << 30. */
static int pixel(const oracle_scene* sc, const mm_uniform* uni, uint32_t px, uint32_t py, uint32_t mirror_limit,
                 float nd[4], float al[4], uint32_t* id) {
    v3 ori = ld3(uni->cam.center), dir = primary_dir(uni, px, py);
    uint32_t mh = 0;
    float dist = 0.0f;
    nd[0] = nd[1] = nd[2] = 0.0f; nd[3] = BIG;
    al[0] = al[1] = al[2] = 0.0f;
    for (;;) {
        float t;
        uint32_t k;
        const int rc = query(sc, ori, dir, &t, &k);
        if (rc || k == AOV_MISS) {
            al[3] = (float)mh;
            *id = k;
            return rc;
        }
        const mm_rect* r = &sc->rects[k];
        const v3 nn = normalize3(cross3(ld3(r->v), ld3(r->u)));
        const float sg = msign(dot3(dir, nn));
        const float side = -sg;
        dist = dist + t;
        const int lit = sc->is_mirror[k] == 0 || sg == 1.0f;
        if (lit || !(mh + 1 < mirror_limit)) {
            const v3 n = vscale(side, nn);
            nd[0] = n.x; nd[1] = n.y; nd[2] = n.z; nd[3] = dist;
            al[0] = r->color[0]; al[1] = r->color[1]; al[2] = r->color[2]; al[3] = (float)mh;
            *id = k | (lit ? 1u << 30 : 2u << 30);
            return MM_OK;
        }
        ori = vadd(ori, vscale(t, dir));                      /* %391 */
        const float dd = dot3(nn, dir) * 2.0f;                /* %392-%393 */
        const v3 rf = vsub(dir, vscale(dd, nn));              /* %397 reflect */
        dir = vscale(rsq(dot3(rf, rf)), rf);                  /* %402 */
        mh = mh + 1;
    }
}

int aovref_pixel(const oracle_scene* sc, const mm_uniform* uni, uint32_t px, uint32_t py, uint32_t mirror_limit,
                 float nd[4], float al[4], uint32_t* id) {
    const unsigned saved = fp_enter();
    const int rc = pixel(sc, uni, px, py, mirror_limit, nd, al, id);
    fp_leave(saved);
    return rc;
}

/* aovref_pixel over the tile (x0 + i, y0 + j * y_stride): nd, al w*h*4 floats, id w*h words */
int aovref_tile(const oracle_scene* sc, const mm_uniform* uni, uint32_t mirror_limit, uint32_t x0, uint32_t y0,
                uint32_t w, uint32_t h, uint32_t y_stride, float* nd, float* al, uint32_t* id) {
    int rc = MM_OK;
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const size_t p = (size_t)j * w + i;
            const int r = aovref_pixel(sc, uni, x0 + i, y0 + j * y_stride, mirror_limit, nd + 4 * p, al + 4 * p,
                                       id + p);
            if (r) rc = r;
        }
    return rc;
}
