// C restatement of rewritten forms of the trace kernel's bounce block and
// chunk prologue next to the forms they replace.  In the kernel: the walk's
// start cell clamped in float (csrc/mm_grid.h grid_first_f) and shade_step's
// shared tail and side test (mm_trace.h).  Checked here but not in the kernel
// (the ISA census showed no gain): msign and rsq's range test
// on the bits, the chunk prologue's pix / w by reciprocal and correction.
// Each function runs both forms over its inputs and returns the number of
// inputs on which they differ in any bit.  Compiled by
// tests/test_bounce_identities.py with -ffp-contract=off.
#include <math.h>
#include <stdint.h>
#include <string.h>

static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---- msign ------------------------------------------------------------------
static float msign_old(float x) {
    if (x > 0.0f) return 1.0f;
    if (x < 0.0f) return -1.0f;
    if (x != x) return 0.0f;
    return x;
}
static float msign_new(float x) {
    const uint32_t b = f2u(x), m = b & 0x7FFFFFFFu;
    const uint32_t one = (b & 0x80000000u) | 0x3F800000u;
    return u2f(m - 1u < 0x7F800000u ? one : (m ? 0u : b));
}
uint64_t bi_msign(const uint32_t* bits, uint64_t n) {
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float x = u2f(bits[i]);
        bad += f2u(msign_old(x)) != f2u(msign_new(x));
        bad += (msign_old(x) == 1.0f) != (x > 0.0f);  // shade_step's side test reads dn itself
    }
    return bad;
}

// ---- rsq's range predicate ----------------------------------------------------
static int rsq_fast_old(float x) { return x >= 0x1p-40f && x <= 0x1p40f; }
static int rsq_fast_new(float x) { return f2u(x) - 0x2B800000u <= 0x53800000u - 0x2B800000u; }
uint64_t bi_rsq_range(const uint32_t* bits, uint64_t n, uint64_t* n_fast) {
    uint64_t bad = 0, fast = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float x = u2f(bits[i]);
        bad += rsq_fast_old(x) != rsq_fast_new(x);
        fast += rsq_fast_new(x) != 0;
    }
    *n_fast = fast;
    return bad;
}

// ---- the walk's start cell ----------------------------------------------------
// The device's float -> int convert saturates and sends NaN to 0.
static int cvt_i32(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return (-2147483647 - 1);
    return (int)f;
}
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }
// per input: (o, mn, inv, nm1) and the two signs of y; compared: the cell
// index, and the boundary index as the float the crossing time's fma reads
uint64_t bi_first_cell(const float* o, const float* mn, const float* inv, const int32_t* nm1, uint64_t n,
                       uint64_t* n_clamped) {
    uint64_t bad = 0, clamped = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const float v = (o[k] - mn[k]) * inv[k];
        const int raw = cvt_i32(floorf(v));
        const int i_old = imin(imax(raw, 0), nm1[k]);
        clamped += raw != i_old;
        // (the kernel's median of three is this min / max for every non-NaN v; NaN gives 0 by both)
        const float f_new = fminf(fmaxf(floorf(v), 0.0f), (float)nm1[k]);
        for (int up = 0; up < 2; ++up) {
            const int b_old = up ? i_old + 1 : i_old;           // grid_first
            const float fb_old = (float)b_old;
            const int ix_old = up ? b_old - 1 : b_old;
            const float fb_new = f_new + (up ? 1.0f : 0.0f);
            const int ix_new = cvt_i32(f_new);
            bad += f2u(fb_old) != f2u(fb_new) || ix_old != ix_new;
        }
    }
    *n_clamped = clamped;
    return bad;
}

// ---- the chunk prologue's pix / w ----------------------------------------------
// rw_ulps: the reciprocal estimate is the correctly rounded 1 / w moved by that
// many ulps (the hardware's is within one).
uint64_t bi_pix_div(uint32_t w, uint32_t lo, uint32_t hi, int rw_ulps) {
    const float rw = u2f(f2u(1.0f / (float)w) + (uint32_t)rw_ulps);
    uint64_t bad = 0;
    for (uint32_t pix = lo; pix < hi; ++pix) {
        const uint32_t q = (uint32_t)((float)pix * rw);
        const int r = (int)pix - (int)((q & 0xFFFFFFu) * (w & 0xFFFFFFu));
        const uint32_t j = q + (r >= (int)w ? 1u : 0u) - (r < 0 ? 1u : 0u);
        const uint32_t i = pix - (j & 0xFFFFFFu) * (w & 0xFFFFFFu);
        bad += j != pix / w || i != pix % w;
    }
    return bad;
}
// path >> log2(spp) for a power of two
uint64_t bi_spp_shift(uint32_t spp, uint32_t lo, uint32_t hi) {
    uint64_t bad = 0;
    for (uint32_t path = lo; path < hi; ++path) bad += (path >> __builtin_ctz(spp)) != path / spp;
    return bad;
}

// ---- shade_step's shared tail ---------------------------------------------------
static float dot3(const float* a, const float* b) {
    float s = a[0] * b[0];
    s = s + a[1] * b[1];
    return s + a[2] * b[2];
}
// dir, nn, rn: 3 floats per input.  Old: the mirror's x = dir - (dot(nn, dir) * 2) nn and the diffuse
// x = rn + (-sign(dot(dir, nn))) nn; new: dn = dot(dir, nn) once, x = base + c nn.
uint64_t bi_tail(const float* dir, const float* nn, const float* rn, uint64_t n) {
    uint64_t bad = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const float *d = dir + 3 * k, *m = nn + 3 * k, *r = rn + 3 * k;
        const float dn = dot3(d, m);
        const float dd = dot3(m, d) * 2.0f;
        const float side = -msign_old(dot3(d, m));
        const float c_m = -(dn * 2.0f), c_d = -msign_new(dn);
        for (int a = 0; a < 3; ++a) {
            const float xm_old = d[a] - dd * m[a], xd_old = r[a] + side * m[a];
            const float xm_new = d[a] + c_m * m[a], xd_new = r[a] + c_d * m[a];
            bad += f2u(xm_old) != f2u(xm_new) || f2u(xd_old) != f2u(xd_new);
        }
    }
    return bad;
}
