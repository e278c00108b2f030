/*
 * aov_ref.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of mm_query_rays and
 * mm_trace_aov (include/mm_api.h), built from the oracle's own functions the
 * way oracle/grid_cpu.c builds on them.  tests/test_aov.py and
 * tests/test_gpu_aov.py compile it into a temporary directory with the oracle
 * Makefile's CFLAGS.
 *
 * Two builds (tests/aov_support.py build_ref):
 *   plain             over the reference walk, which can record its queries
 *                     (aovref_record: tests/test_grid_stress.py states its
 *                     input conditions on the recorded chains);
 *   -DAOVREF_TWIN     over oracle/grid_cpu.c, the CPU twin of the certified grid
 *                     search: the same entry points answer with the search and
 *                     its walk fallback (gridcpu_build / gridcpu_stats exported).
 */
#ifdef AOVREF_TWIN
#include "../oracle/grid_cpu.c"
#define AOV_WALK grid_query_or_walk
#else
#define ORACLE_QUERY_FN recorded_walk
#include "../oracle/mm_oracle.c"
#define AOV_WALK recorded_walk

/* Every query of the calling thread while a buffer is set: 8 floats per query,
 * (o.xyz, t, d.xyz, bits of k) with (1e30, AOV_MISS) for a miss. */
static __thread float* g_rec;
static __thread uint64_t g_rec_cap, g_rec_n;

static void recorded_walk(ray_t* b, const oracle_scene* sc, trav_t* tr) {
    const float t0 = b->t;
    intersect_bvh(b, sc, tr);
    if (!g_rec) return;
    if (g_rec_n < g_rec_cap) {
        float* q = g_rec + 8 * g_rec_n;
        const uint32_t k = b->t < t0 ? b->index : 0xFFFFFFFFu;
        q[0] = b->ori.x; q[1] = b->ori.y; q[2] = b->ori.z; q[3] = b->t;
        q[4] = b->dir.x; q[5] = b->dir.y; q[6] = b->dir.z;
        memcpy(q + 7, &k, 4);
    }
    ++g_rec_n;
}

/* Start recording into rec (cap queries of 8 floats); rec = NULL stops.
 * Returns the number of queries seen since the last start (may exceed cap). */
uint64_t aovref_record(float* rec, uint64_t cap) {
    const uint64_t n = g_rec_n;
    g_rec = rec; g_rec_cap = cap; g_rec_n = 0;
    return n;
}
#endif

#define AOV_MISS 0xFFFFFFFFu
#define AOV_FAILED 0xFFFFFFFEu

/* The (t, k) intersect_bvh_iterative ends with when started at t = 1e30
 * (k starts as AOV_MISS, which a miss leaves).  Returns 0, or MM_ERR_STACK
 * with (1e30, AOV_FAILED). */
static int query(const oracle_scene* sc, v3 o, v3 d, float* t, uint32_t* k) {
    ray_t b;
    trav_t tr = {0, 0, 0};
    b.ori = o; b.dir = d; b.t = BIG; b.index = AOV_MISS;
    AOV_WALK(&b, sc, &tr);
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

/* ---- the grid walk's crossing times (tests/test_grid_stress.py, case C) -------
 * A float32 restatement of the certified search's cell walk (mm_grid.h
 * grid_search): per axis A = RN(RN(mn - o) * y), B = RN(cell * y), y = RN(1 / d),
 * and the crossing time of boundary b is fmaf(b, B, A); the walk starts in the
 * cell of the ray's point at t = 3/32 and steps the axis whose time comes first
 * (x before y before z on equal times).  g = mn.xyz, cell.xyz, n.xyz (as
 * floats), mx.xyz.  best[i]: the reference's hit distance of ray i (1e30: a
 * miss), which ends the walk.
 *   flat = 1  the maze forms' walk: x and z steps while te <= best and te < tend,
 *             tend = min(ty, the time of the last x boundary, of the last z one);
 *   flat = 0  the 3-D walk: steps while best >= te and the boundary index stays
 *             inside 0..n.
 * out[0] steps taken with tx == tz == te; out[1] rays whose walk ended at
 * te == tend (flat) or by leaving the grid (3-D); out[2] cells entered through an
 * interior x or z boundary at the instant the ray leaves the grid through the
 * other of the two (the 3-D walk tests such a cell, the maze forms end before
 * it); out[3] rays walked (inside the box and the direction guards); out[4] steps.
 * flags (or NULL): per ray, bit 0 a tied step, bit 1 ended at tend / left the grid,
 * bit 2 a cell entered at the exit instant. */
static int walk_first(const float* g, int a, float o, float y) {
    int i = (int)floorf((o - g[a]) * (1.0f / g[3 + a]));
    const int nm1 = (int)g[6 + a] - 1;
    if (i < 0) i = 0;
    if (i > nm1) i = nm1;
    return y > 0.0f ? i + 1 : i;
}

void aovref_walk_ties(const float* g, int flat, const float* rays, uint64_t n, const float* best, uint64_t out[5],
                      uint8_t* flags) {
    const unsigned saved = fp_enter();
    for (int i = 0; i < 5; ++i) out[i] = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const float* o = rays + 8 * r;
        const float* d = rays + 8 * r + 4;
        int ok = 1;
        for (int a = 0; a < 3; ++a) {
            const float ad = fabsf(d[a]);
            ok &= ad >= 0x1p-40f && ad <= 0x1p40f && o[a] >= g[a] && o[a] <= g[9 + a];
        }
        if (flags) flags[r] = 0;
        if (!ok) continue;
        out[3]++;
        const uint64_t before[3] = {out[0], out[1], out[2]};
        float y[3], A[3], B[3], t[3], tl[3], last[3];
        int b[3], st[3];
        for (int a = 0; a < 3; ++a) {
            y[a] = 1.0f / d[a];
            st[a] = y[a] > 0.0f ? 1 : -1;
            A[a] = (g[a] - o[a]) * y[a];
            B[a] = g[3 + a] * y[a];
            b[a] = walk_first(g, a, o[a] + 0.09375f * d[a], y[a]);
            t[a] = fmaf((float)b[a], B[a], A[a]);
            last[a] = y[a] > 0.0f ? g[6 + a] : 0.0f;  /* the boundary the ray leaves the grid through */
            tl[a] = fmaf(last[a], B[a], A[a]);
        }
        if (flat) {
            b[1] = y[1] > 0.0f ? 1 : 0;
            t[1] = ((g[1] + (float)b[1] * g[4]) - o[1]) * y[1];
            const float tend = fminf(t[1], fminf(tl[0], tl[2]));
            for (;;) {
                const int a = t[0] <= t[2] ? 0 : 2;
                const float te = t[a];
                if (!(te <= best[r]) || !(te < tend)) {
                    if (te == tend) {
                        out[1]++;
                        if (te <= best[r] && (float)b[a] != last[a]) out[2]++;
                    }
                    break;
                }
                if (t[0] == t[2]) out[0]++;
                out[4]++;
                b[a] += st[a];
                t[a] = fmaf((float)b[a], B[a], A[a]);
            }
        } else {
            for (;;) {
                const float te = fminf(t[0], fminf(t[1], t[2]));
                if (best[r] < te) break;
                const int a = t[0] == te ? 0 : (t[1] == te ? 1 : 2);
                const int c = a == 0 ? 2 : 0;
                const int tied = t[0] == t[2] && t[0] == te;
                if ((float)b[a] == last[a]) {  /* this step leaves the grid */
                    out[1]++;
                    break;
                }
                if (tied) out[0]++;
                if (a != 1 && t[c] == te && (float)b[c] == last[c]) out[2]++;
                out[4]++;
                b[a] += st[a];
                t[a] = fmaf((float)b[a], B[a], A[a]);
            }
        }
        if (flags) flags[r] = (out[0] > before[0]) | (out[1] > before[1]) << 1 | (out[2] > before[2]) << 2;
    }
    fp_leave(saved);
}

