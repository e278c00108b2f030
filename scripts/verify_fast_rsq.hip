// verify_fast_rsq.hip — exhaustive GPU checks of the exact fast forms of two
// IEEE operations on the path, compiled with the product library's flags
// (built by mirror-maze_amd/Makefile into lib/verify_fast_rsq, run by
// tests/test_gpu_arith.py):
//   rsq          mm::rsq (mm_device.h: hardware sqrt / rcp with exact
//                corrections on [2^-40, 2^40]) against the IEEE expansion
//                1.0f / sqrtf(x) -- the reference's fast_rsqrt with its IEEE
//                meaning -- for EVERY float x in [2^-44, 2^44] (the range and
//                4 binades either side, which take the IEEE path);
//   rcp_guarded  mm::rcp_guarded (mm_trace.h: one fma Newton step on v_rcp_f32,
//                the per-ray y = RN(1/d) the Markstein quotients read) against
//                1.0f / d for EVERY float d of either sign with |d| in
//                [2^-40, 2^40] (the guard's range; outside it y is never read);
//   ray_guard    mm::ray_fast_ok_boxed (mm_trace.h: the per-query guard in
//                integer form) against mm::ray_fast_ok for EVERY 32-bit
//                pattern on one axis of the direction (the others 1), and on
//                one axis of the origin wherever the grid box check can pass
//                (|o| <= 2^60, not NaN; grid_build.cpp builds no grid past it).
// and, against values computed in this program's host code (check_against_host),
// over 4100 mantissas in every binade from the smallest denormal to the largest
// finite float, +-0, +-inf and NaN:
//   ieee_sqrt, ieee_rsq   the device's sqrtf(x) and mm::rsq(x) -- rsq_ieee
//                outside [2^-40, 2^40] -- against the host's sqrtf(x) and
//                1.0f / sqrtf(x);
//   ieee_div     the device's a / d, d over every binade and a over the
//                exponents -126..127, against the host's a / d;
//   ieee_div_markstein    mm::qdiv(a, d, mm::rcp_guarded(d)) inside the guarded
//                ranges, a nonzero, against the host's a / d
//                (scripts/verify_markstein.c's claim, there with the host's
//                fmaf);
//   markstein_zero        the same for a = +-0: the host's zero, but +0 for
//                a = -0 over d > 0 (mm_trace.h qdiv);
//   cvt_u32_sat, unorm8   against host restatements around 0, 2^32, the
//                0.5 / 255 ties, NaN and +-inf;
//   host_ref     the host's float results against the double-precision route.
// Prints one line per check:  <name> checked <n> mismatches <m> [first 0x<bits>]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "mm_trace.h"

template <int kWhich>
__global__ void k_check(uint32_t lo, uint32_t hi, unsigned long long* bad, uint32_t* first) {
    const uint64_t n = (uint64_t)hi - lo + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = lo + (uint32_t)i;
        const float x = __uint_as_float(b);
        bool diff;
        if constexpr (kWhich == 0) {
            diff = __float_as_uint(mm::rsq(x)) != __float_as_uint(mm::rsq_ieee(x));
        } else if constexpr (kWhich == 2) {
            mm::Ray rd{}, ro{};
            rd.o = mm::F3{1.0f, 1.0f, 1.0f};
            rd.d = mm::F3{1.0f, x, 1.0f};
            ro.o = mm::F3{1.0f, 1.0f, x};
            ro.d = mm::F3{1.0f, 1.0f, 1.0f};
            diff = mm::ray_fast_ok_boxed(rd) != mm::ray_fast_ok(rd);
            if (!(fabsf(x) > 0x1p60f) && x == x) diff |= mm::ray_fast_ok_boxed(ro) != mm::ray_fast_ok(ro);
        } else {
            const float a = mm::rcp_guarded(x), e = 1.0f / x;
            const float an = mm::rcp_guarded(-x), en = 1.0f / -x;
            diff = __float_as_uint(a) != __float_as_uint(e) || __float_as_uint(an) != __float_as_uint(en);
        }
        if (diff) {
            atomicAdd(bad, 1ull);
            atomicMin(first, b);
        }
    }
}

template <int kWhich>
static int check_bits(const char* name, uint32_t lo, uint32_t hi, unsigned long long* bad, uint32_t* first) {
    (void)hipMemset(bad, 0, 8);
    (void)hipMemset(first, 0xFF, 4);
    hipLaunchKernelGGL(k_check<kWhich>, dim3(65536), dim3(256), 0, 0, lo, hi, bad, first);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    unsigned long long h_bad = 0;
    uint32_t h_first = 0;
    (void)hipMemcpy(&h_bad, bad, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&h_first, first, 4, hipMemcpyDeviceToHost);
    printf("%s checked %llu mismatches %llu", name, (unsigned long long)hi - lo + 1, h_bad);
    if (h_bad) printf(" first 0x%08x", h_first);
    printf("\n");
    return h_bad ? 1 : 0;
}
template <int kWhich>
static int check(const char* name, float lo_f, float hi_f, unsigned long long* bad, uint32_t* first) {
    uint32_t lo, hi;
    memcpy(&lo, &lo_f, 4);
    memcpy(&hi, &hi_f, 4);
    return check_bits<kWhich>(name, lo, hi, bad, first);
}

// ---- device results against values computed on the host ------------------------
// The rows above compare two device computations.  These compare the device's
// IEEE operations, and the fast forms over a sample of all binades, with the
// host's: a / d, sqrtf(x) and 1.0f / sqrtf(x) in float, each cross-checked on
// the host against the double-precision route rounded once to float (exact for
// both operations at 24 bits: a 53-bit quotient or root of 24-bit operands is
// never a rounding tie of a shorter format unless it is exact) -- the host_ref row.
constexpr uint32_t kRandomMantissas = 4096;

static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 11); }

// Mantissas per binade: 0, 1, 0x7FFFFF, 0x7FFFFE and kRandomMantissas seeded ones.
static std::vector<uint32_t> mantissa_sample() {
    std::vector<uint32_t> m = {0u, 1u, 0x7FFFFFu, 0x7FFFFEu};
    for (uint32_t i = 0; i < kRandomMantissas; ++i) m.push_back(rnd() & 0x7FFFFFu);
    return m;
}
// Positive floats of the binades [first, last]: binade 0..22 are the denormal
// ones, [2^(b-149), 2^(b-148)) (the top b bits of each sampled mantissa: the
// binade has 2^b patterns), binade 22 + e the normal one with exponent field e
// (1..254).
static void add_binades(std::vector<uint32_t>& out, const std::vector<uint32_t>& ms, int first, int last) {
    for (int b = first; b <= last; ++b)
        for (uint32_t m : ms) out.push_back(b < 23 ? (1u << b) + (m >> (23 - b)) : ((uint32_t)(b - 22) << 23) | m);
}
constexpr int kBinades = 23 + 254;
static const uint32_t kSpecials[] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7F800001u,
                                     0xBF800000u, 0x80000001u};  // +-0, +-inf, two NaNs, -1, a negative denormal

enum { kOpSqrt, kOpRsq, kOpCvt, kOpUnorm };
template <int kOp>
__global__ void k_unary(const uint32_t* __restrict__ x, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = __uint_as_float(x[i]);
    if constexpr (kOp == kOpSqrt) out[i] = __float_as_uint(sqrtf(v));
    else if constexpr (kOp == kOpRsq) out[i] = __float_as_uint(mm::rsq(v));
    else if constexpr (kOp == kOpCvt) out[i] = mm::cvt_u32_sat(v);
    else out[i] = mm::unorm8(v);
}
template <bool kMarkstein>
__global__ void k_div(const uint32_t* __restrict__ a, const uint32_t* __restrict__ d, uint32_t* __restrict__ out,
                      uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float av = __uint_as_float(a[i]), dv = __uint_as_float(d[i]);
    out[i] = __float_as_uint(kMarkstein ? mm::qdiv(av, dv, mm::rcp_guarded(dv)) : av / dv);
}

struct DevWords {
    uint32_t* p = nullptr;
    explicit DevWords(const std::vector<uint32_t>& h) {
        if (hipMalloc(&p, h.size() * 4 + 4) == hipSuccess) (void)hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    }
    explicit DevWords(size_t n) { (void)hipMalloc(&p, n * 4 + 4); }
    ~DevWords() { (void)hipFree(p); }
};
static bool fetch(const DevWords& d, std::vector<uint32_t>& h) {
    return hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), d.p, h.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
}
static bool is_nan_bits(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }
// One row: got[i] against want[i] (as floats: two NaNs agree), `in` the first operand for the report.
static int report(const char* name, const std::vector<uint32_t>& in, const std::vector<uint32_t>& got,
                  const std::vector<uint32_t>& want, bool floats) {
    unsigned long long bad = 0;
    size_t first = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        const bool same = got[i] == want[i] || (floats && is_nan_bits(got[i]) && is_nan_bits(want[i]));
        if (!same && !bad++) first = i;
    }
    printf("%s checked %llu mismatches %llu", name, (unsigned long long)got.size(), bad);
    if (bad) printf(" first 0x%08x got 0x%08x want 0x%08x", in[first], got[first], want[first]);
    printf("\n");
    return bad ? 1 : 0;
}

static float host_div(float a, float d) { volatile float x = a, y = d; return x / y; }
static float host_sqrt(float x) { volatile float v = x; return sqrtf(v); }
static float host_rsq(float x) { volatile float s = host_sqrt(x); return 1.0f / s; }
// air.convert.u.i32.f.f32 restated over double: truncation, saturating, NaN -> 0
static uint32_t host_cvt_u32_sat(float f) {
    const double d = f;
    if (!(d > 0.0)) return 0u;
    return d >= 4294967296.0 ? 0xFFFFFFFFu : (uint32_t)(uint64_t)d;
}
// RGBA8Unorm restated: the float product with 255, rounded to nearest even by hand (p < 2^8: p - floor(p) is exact)
static uint32_t host_unorm8(float x) {
    const float c = x != x ? 0.0f : (x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x));
    volatile float p = c * 255.0f;
    const float fl = floorf(p), fr = p - fl;
    uint32_t k = (uint32_t)fl;
    if (fr > 0.5f || (fr == 0.5f && (k & 1u))) ++k;
    return k;
}

template <typename K>
static bool run(K kernel, const std::vector<uint32_t>& x, std::vector<uint32_t>& out) {
    DevWords dx(x), dout(x.size());
    out.assign(x.size(), 0u);
    if (!dx.p || !dout.p) return false;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((x.size() + 255) / 256)), dim3(256), 0, 0, dx.p, dout.p, (uint32_t)x.size());
    return fetch(dout, out);
}
template <typename K>
static bool run2(K kernel, const std::vector<uint32_t>& a, const std::vector<uint32_t>& d, std::vector<uint32_t>& out) {
    DevWords da(a), dd(d), dout(a.size());
    out.assign(a.size(), 0u);
    if (!da.p || !dd.p || !dout.p) return false;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((a.size() + 255) / 256)), dim3(256), 0, 0, da.p, dd.p, dout.p,
                       (uint32_t)a.size());
    return fetch(dout, out);
}

static int check_against_host() {
    const std::vector<uint32_t> ms = mantissa_sample();
    unsigned long long host_n = 0, host_bad = 0;
    auto host_agree = [&](float f, double via_double) {
        const uint32_t a = f2u(f), b = f2u((float)via_double);
        ++host_n;
        if (a != b && !(is_nan_bits(a) && is_nan_bits(b))) ++host_bad;
    };
    int rc = 0;
    std::vector<uint32_t> got, want;
    // ieee_sqrt, ieee_rsq: every binade from the smallest denormal to the largest finite float, and the specials
    std::vector<uint32_t> x;
    add_binades(x, ms, 0, kBinades - 1);
    x.insert(x.end(), kSpecials, kSpecials + sizeof(kSpecials) / 4);
    want.resize(x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        const float v = u2f(x[i]), s = host_sqrt(v);
        want[i] = f2u(s);
        host_agree(s, sqrt((double)v));
    }
    if (!run(k_unary<kOpSqrt>, x, got)) return 3;
    rc |= report("ieee_sqrt", x, got, want, true);
    for (size_t i = 0; i < x.size(); ++i) {
        const float v = u2f(x[i]), q = host_rsq(v);
        want[i] = f2u(q);
        host_agree(q, 1.0 / (double)host_sqrt(v));
    }
    if (!run(k_unary<kOpRsq>, x, got)) return 3;
    rc |= report("ieee_rsq", x, got, want, true);
    // ieee_div: d over the same sample with either sign, two a per d: exponents -126..127, the same mantissas
    std::vector<uint32_t> a, d;
    for (uint32_t xb : x)
        for (int j = 0; j < 2; ++j) {
            d.push_back(xb ^ (rnd() & 1u ? 0x80000000u : 0u));
            a.push_back(((rnd() & 1u) << 31) | ((1u + rnd() % 254u) << 23) | ms[rnd() % ms.size()]);
        }
    want.resize(a.size());
    for (size_t i = 0; i < a.size(); ++i) {
        const float q = host_div(u2f(a[i]), u2f(d[i]));
        want[i] = f2u(q);
        host_agree(q, (double)u2f(a[i]) / (double)u2f(d[i]));
    }
    if (!run2(k_div<false>, a, d, got)) return 3;
    rc |= report("ieee_div", d, got, want, true);
    // ieee_div_markstein: qdiv(a, d, rcp_guarded(d)) inside the guarded ranges -- |d| in [2^-40, 2^40] and
    // |a| in [2^-53, 2^61] (a nonzero difference of two coordinates that are 0 or in [2^-30, 2^60]: mm_runtime.hip
    // coord_ok, mm_trace.h org_ok), four a per d
    std::vector<uint32_t> dg;
    add_binades(dg, ms, 22 + 127 - 40, 22 + 127 + 39);
    dg.push_back(f2u(0x1p40f));
    a.clear();
    d.clear();
    for (uint32_t xb : dg)
        for (int j = 0; j < 4; ++j) {
            d.push_back(xb ^ (rnd() & 1u ? 0x80000000u : 0u));
            a.push_back(((rnd() & 1u) << 31) | ((uint32_t)(127 - 53 + (int)(rnd() % 114u)) << 23) | ms[rnd() % ms.size()]);
        }
    want.resize(a.size());
    for (size_t i = 0; i < a.size(); ++i) {
        const float q = host_div(u2f(a[i]), u2f(d[i]));
        want[i] = f2u(q);
        host_agree(q, (double)u2f(a[i]) / (double)u2f(d[i]));
    }
    if (!run2(k_div<true>, a, d, got)) return 3;
    rc |= report("ieee_div_markstein", d, got, want, true);
    // markstein_zero: a = +-0 (a bound equal to the origin's coordinate) over the same d of either sign.  The
    // quotient is the zero RN(a / d) is, except that a = -0 over d > 0 gives +0 where IEEE gives -0: r = fma(-q, d, a)
    // adds zeros of opposite signs, +0, and fma(+0, y, -0) = +0 for y > 0 (mm_trace.h qdiv says why no caller can tell).
    a.clear();
    d.clear();
    for (uint32_t xb : dg)
        for (uint32_t sa : {0u, 0x80000000u})
            for (uint32_t sd : {0u, 0x80000000u}) {
                a.push_back(sa);
                d.push_back(xb | sd);
            }
    want.resize(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        want[i] = a[i] == 0x80000000u && !(d[i] >> 31) ? 0u : f2u(host_div(u2f(a[i]), u2f(d[i])));
    if (!run2(k_div<true>, a, d, got)) return 3;
    rc |= report("markstein_zero", d, got, want, false);
    // cvt_u32_sat, unorm8: the values around 0, 2^32, the 0.5 / 255 ties, NaN and +-inf
    x.assign(kSpecials, kSpecials + sizeof(kSpecials) / 4);
    for (float v : {0x1p-149f, 0x1p-126f, 0.5f, 0x1.fffffep-1f, 1.0f, 0x1.000002p0f, 1.5f, 2.5f, 255.0f, 0x1.fffffep30f,
                    0x1p31f, 0x1.000002p31f, 0x1.fffffep31f, 0x1p32f, 0x1.000002p32f, 0x1p33f, 1e30f, 0x1.fffffep127f})
        for (float sg : {1.0f, -1.0f}) x.push_back(f2u(sg * v));
    for (int k = 0; k < 256; ++k)
        for (double off : {0.0, 0.5})
            for (int du = -2; du <= 2; ++du) x.push_back(f2u((float)((k + off) / 255.0)) + (uint32_t)du);
    want.resize(x.size());
    for (size_t i = 0; i < x.size(); ++i) want[i] = host_cvt_u32_sat(u2f(x[i]));
    if (!run(k_unary<kOpCvt>, x, got)) return 3;
    rc |= report("cvt_u32_sat", x, got, want, false);
    for (size_t i = 0; i < x.size(); ++i) want[i] = host_unorm8(u2f(x[i]));
    if (!run(k_unary<kOpUnorm>, x, got)) return 3;
    rc |= report("unorm8", x, got, want, false);
    printf("host_ref checked %llu mismatches %llu\n", host_n, host_bad);
    return rc | (host_bad ? 1 : 0);
}

int main() {
    unsigned long long* bad = nullptr;
    uint32_t* first = nullptr;
    if (hipMalloc(&bad, 8) != hipSuccess || hipMalloc(&first, 4) != hipSuccess) return 2;
    int rc = check<0>("rsq", 0x1p-44f, 0x1p44f, bad, first);
    rc |= check<1>("rcp_guarded", 0x1p-40f, 0x1p40f, bad, first);
    rc |= check_bits<2>("ray_guard", 0u, 0xFFFFFFFFu, bad, first);
    rc |= check_against_host();
    return rc;
}
