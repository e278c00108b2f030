// denoise_kernels.hip — the edge-aware a-trous filter of mm_denoise_frames and its
// variance-guided form, mm_denoise_frames_var (include/mm_api.h states the arithmetic;
// tests/denoise_ref.c and tests/denoise_var_ref.c restate it in plain C and the GPU
// result, colour and variance, equals them bit for bit).  One source for both calls:
// the pass kernel and the two pixel forms are templates over kVar, and what the
// variance call adds stands under `if constexpr (kVar)`.
//
//   k_denoise_keys  once per call: (id, al.w) of every pixel as one 8-byte
//                   record, so a tap's key test reads 8 B in one load instead
//                   of 4 B + a 4-byte word out of a 16-byte stride (measured:
//                   0.41 against 0.50 ms per frame of four passes).
//   k_denoise_pass  one pass: one thread per output pixel, 64 x 4 blocks, so a
//                   wave is a 64-pixel row segment and each of its 25 taps is
//                   one coalesced row segment of the input (taps 2^pass apart).
//                   The taps are accumulated one after the other in the order
//                   of the specification (dy outer, dx inner): no tree, no
//                   contraction (-ffp-contract=off).  The last pass may store
//                   RGBA8 (unorm8 of its float result, as k_quantize).
//
// A taken tap is four divisions (two soft terms, a quotient and a weight each),
// and 25 taps of the compiler's IEEE sequence (~12 operations per division)
// made the pass VALU-bound at 0.143 ms per 1080p pass (profiles/denoise/ab.txt).
// So a pixel is computed twice over, if need be:
//   fast   straight-line code, no branch: tap addresses are clamped into the
//          frame, so every load is unconditional and in bounds, and a tap
//          row's 15 loads are issued ahead of its arithmetic; a tap outside
//          the frame or rejected by the key test is computed and not added
//          (a select, not a zero weight: the accumulators never see it).
//          Quotients are Markstein's over a correctly rounded reciprocal
//          (dn_div, mm_denoise.h, 6 operations), which are RN(a / d) inside exponent
//          ranges that a taken tap's operands leave only for odd inputs.
//   exact  where some taken tap of the pixel was outside those ranges, the
//          pixel is computed again by a plain loop with IEEE division, and
//          that result is stored.
//
// The variance pass (kVar; mm_denoise_frames_var) is laid out as the plain one: one
// thread per output pixel, 64 x 4 blocks, a wave per 64-pixel row segment, the packed
// (id, al.w) keys of k_denoise_keys, taps accumulated one after the other in the order
// of the specification, no contraction.  Beside the colour it carries the variance of
// the pixel mean: a tap adds (g * g) * V_q, and the pass writes SV / (W * W) to a
// float image of its own.
//
// What differs from the plain pass:
//   the stop   With the luminance term on, a pixel's stop slp comes from a 3 x 3 of
//              the pass's input variance around it (unit spacing in every pass, the
//              same surface test as the taps).  Its 9 taps are branch-free as the
//              25 are (clamped addresses, a select per tap); GV / GW and sqrtf are
//              the compiler's IEEE forms, once per pixel.  slp is then the one
//              denominator of the pixel's 25 luminance quotients: its guarded
//              reciprocal and its dn_den_ok test are taken once per pixel.  (The
//              plain pass's denominator is a.sl, the same for every pixel.)
//   fast/exact As in the plain pass: the straight-line form with Markstein
//              quotients, and, where a taken tap left their ranges (a stop below
//              2^-40, a factor above 2^40, ...), the pixel again by a plain loop
//              with IEEE division.  Both forms take slp from the same code.
//
// Subnormals.  A weight g can be as small as 2^-88, so g * g and (g * g) * V_q can be
// subnormal or zero, and V itself may hold subnormals; the reference is plain C with
// IEEE subnormals.  The library is built without -fgpu-flush-denormals-to-zero, so
// the kernels run with f32 denormals kept on both inputs and results
// (float_denorm_mode_32 = 3 in the kernel descriptor), and v_mul_f32, v_add_f32, the
// IEEE division sequence and sqrtf round such values as the host does.  The products
// and sums of the variance are therefore plain C++ in the fast form too: no range
// test guards them and no pixel goes to the exact form on their account.  (The
// hardware reciprocal does flush; it is only ever taken of denominators that
// dn_den_ok has passed, or its result is discarded with the pixel.)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mm_denoise.h"
#include "mm_launch.h"
#include "mm_trace.h"

namespace mm {

namespace {

__global__ void k_denoise_keys(const float4* __restrict__ al, const uint32_t* __restrict__ id,
                               uint2* __restrict__ keys, size_t n) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        keys[i] = make_uint2(id[i], __float_as_uint(al[i].w));
}

// A pass kernel's argument (mm_launch.h): the two structs name what they share alike, and each keeps the layout
// its instances were measured with.
template <bool kVar>
using DnArgs = std::conditional_t<kVar, DnVarPass, DnPass>;

// The stop of pixel c: sigma_l * sqrt of the 3 x 3 (1/4, 1/2, 1/4)^2 mean of V over the centre's surface, + eps_l.
__device__ __forceinline__ float dnv_stop(const DnVarPass& a, const DnPixel& c) {
    constexpr float k3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    float GV = 0.0f, GW = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const uint32_t qy = c.y + (uint32_t)dy;  // (unsigned: below 0 wraps past the frame, as in the taps)
        const bool in_y = qy < a.h;
        const uint32_t row = (in_y ? qy : c.y) * a.w;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t qx = c.x + (uint32_t)dx;
            const bool in_x = qx < a.w;
            const uint32_t q = row + (in_x ? qx : c.x);  // clamped: always a pixel of this frame
            const float Vq = a.vin[q];
            bool take = in_x & in_y;
            if (dx != 0 || dy != 0) take &= dn_same_surface(a, c, q, a.nd[q]);
            const float g = k3[dy + 1] * k3[dx + 1];
            const float nv = GV + g * Vq, nw = GW + g;
            GV = take ? nv : GV;
            GW = take ? nw : GW;
        }
    }
    return a.sigma_l * sqrtf(GV / GW) + a.eps_l;
}

// kZ / kL: the depth / luminance term is on (sigma > 0).  kVar: the variance is carried (vo).
// sl: the denominator of the luminance quotients (kL) -- a.sl, the same for every pixel of the pass, or the
// pixel's stop (kVar, dnv_stop).
// The fast form: returns false if a taken tap left the guarded quotients' ranges (o, vo are then not to be used).
template <bool kZ, bool kL, bool kVar>
__device__ __forceinline__ bool dn_pixel_fast(const DnArgs<kVar>& a, const DnPixel& c, float sl, float4& o,
                                              float& vo) {
    // 1 / sl for the luminance quotients; sl is the same for every tap of the pixel
    const float ysl = kL ? rcp_guarded(sl) : 0.0f;
    const bool sl_ok = dn_den_ok(sl);
    constexpr float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, W = 0.0f, SV = 0.0f;
    uint32_t bad = 0;  // (a VGPR, so that it can go through the barriers below with the sums)
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        // (unsigned: a coordinate below 0 wraps to above 2^32 - 257, one past the frame stays below 2^31 + 256)
        // (the row's addresses hang on cx, cy, which the compiler cannot see through: it would otherwise work
        // out all 75 of the pixel, 150 VGPRs, ahead of the first row)
        uint32_t cx = c.x, cy = c.y;
        asm volatile("" : "+v"(cx), "+v"(cy));
        const uint32_t qy = cy + a.s * (uint32_t)dy;
        const bool in_y = qy < a.h;
        const uint32_t row = (in_y ? qy : cy) * a.w;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const uint32_t qx = cx + a.s * (uint32_t)dx;
            const bool in_x = qx < a.w;
            const uint32_t q = row + (in_x ? qx : cx);  // clamped: always a pixel of this frame
            const float4 Cq = a.in[q];
            const float4 ndq = a.nd[q];
            float Vq = 0.0f;
            if constexpr (kVar) Vq = a.vin[q];
            bool take = in_x & in_y;
            if (dx != 0 || dy != 0) take &= dn_same_surface(a, c, q, ndq);
            float g = hk[dy + 2] * hk[dx + 2];
            bool ok = true;
            if constexpr (kZ) {
                const float az = c.nd.w - ndq.w, dz = a.sigma_z * (c.nd.w + ndq.w);
                bool ok_z = dn_den_ok(dz);
                ok_z &= dn_num_ok(az);
                ok_z |= az == 0.0f;
                ok &= ok_z;
                const float t = dn_div(az, dz);
                const float f = 1.0f + t * t;
                ok &= f <= 0x1p40f;
                g = dn_div(g, f);
            }
            if constexpr (kL) {
                const float al = c.lum - dn_lum(Cq);
                ok &= sl_ok & dn_num_ok(al);
                const float t = qdiv(al, sl, ysl);
                const float f = 1.0f + t * t;
                ok &= f <= 0x1p40f;
                g = dn_div(g, f);
            }
            bad |= (uint32_t)(take & !ok);
            const float nx = Sx + g * Cq.x, ny = Sy + g * Cq.y, nz = Sz + g * Cq.z, nw = W + g;
            float nv = 0.0f;
            if constexpr (kVar) nv = SV + (g * g) * Vq;
            Sx = take ? nx : Sx;
            Sy = take ? ny : Sy;
            Sz = take ? nz : Sz;
            W = take ? nw : W;
            if constexpr (kVar) SV = take ? nv : SV;
        }
        // a row's 15 loads (20 with the variance) may be batched ahead of its arithmetic, not all 75 (100) of the
        // pixel (one basic block is otherwise laid out loads first: 260 VGPRs, or spills under an occupancy
        // bound): the next row's loads stay behind this point, and this row's sums and range tests are done
        // before it
        if constexpr (kVar) asm volatile("" : "+v"(Sx), "+v"(Sy), "+v"(Sz), "+v"(W), "+v"(SV), "+v"(bad) : : "memory");
        else asm volatile("" : "+v"(Sx), "+v"(Sy), "+v"(Sz), "+v"(W), "+v"(bad) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    o = make_float4(Sx / W, Sy / W, Sz / W, c.C.w);
    if constexpr (kVar) vo = SV / (W * W);
    return bad == 0;
}

// The exact form: the specification as it is written, IEEE division, a rolled loop (it runs for few pixels).
template <bool kZ, bool kL, bool kVar>
__device__ __forceinline__ void dn_pixel_exact(const DnArgs<kVar>& a, const DnPixel& c, float sl, float4& o,
                                               float& vo) {
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, W = 0.0f, SV = 0.0f;
#pragma nounroll
    for (int i = 0; i < 25; ++i) {
        const int dy = i / 5 - 2, dx = i % 5 - 2;
        const uint32_t qx = c.x + a.s * (uint32_t)dx, qy = c.y + a.s * (uint32_t)dy;
        if (qx >= a.w || qy >= a.h) continue;
        const uint32_t q = qy * a.w + qx;
        const float4 ndq = a.nd[q];
        if (i != 12 && !dn_same_surface(a, c, q, ndq)) continue;
        const float4 Cq = a.in[q];
        const float ky = dy == 0 ? 3.0f / 8.0f : (dy == 1 || dy == -1 ? 1.0f / 4.0f : 1.0f / 16.0f);
        const float kx = dx == 0 ? 3.0f / 8.0f : (dx == 1 || dx == -1 ? 1.0f / 4.0f : 1.0f / 16.0f);
        float g = ky * kx;
        if constexpr (kZ) {
            const float t = (c.nd.w - ndq.w) / (a.sigma_z * (c.nd.w + ndq.w));
            g = g / (1.0f + t * t);
        }
        if constexpr (kL) {
            const float t = (c.lum - dn_lum(Cq)) / sl;
            g = g / (1.0f + t * t);
        }
        Sx = Sx + g * Cq.x;
        Sy = Sy + g * Cq.y;
        Sz = Sz + g * Cq.z;
        W = W + g;
        if constexpr (kVar) SV = SV + (g * g) * a.vin[q];
    }
    o = make_float4(Sx / W, Sy / W, Sz / W, c.C.w);
    if constexpr (kVar) vo = SV / (W * W);
}

template <bool kZ, bool kL, bool kVar>
__global__ __launch_bounds__(256) void k_denoise_pass(const DnArgs<kVar> a) {
    const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    DnPixel c;
    c.x = tx * 64 + threadIdx.x;  // (tiles_x * 64 < w + 64 <= 2^31 + 63)
    c.y = ty * 4 + threadIdx.y;
    if (c.x >= a.w || c.y >= a.h) return;
    const uint32_t p = c.y * a.w + c.x;
    c.C = a.in[p];
    c.nd = a.nd[p];
    dn_key(a, p, c.id, c.mh);
    c.lum = dn_lum(c.C);
    float sl = 0.0f;
    if constexpr (!kVar) {
        sl = a.sl;
    } else if constexpr (kL) {
        sl = dnv_stop(a, c);
        // the stop's loads and sums are done before the taps' begin: only the stop lives on
        asm volatile("" : "+v"(sl) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    float4 o;
    float vo;
    if (!dn_pixel_fast<kZ, kL, kVar>(a, c, sl, o, vo)) dn_pixel_exact<kZ, kL, kVar>(a, c, sl, o, vo);
    if (a.rgba8)
        reinterpret_cast<uint32_t*>(a.out)[p] =
            unorm8(o.x) | (unorm8(o.y) << 8) | (unorm8(o.z) << 16) | (unorm8(o.w) << 24);
    else
        reinterpret_cast<float4*>(a.out)[p] = o;
    if constexpr (kVar)
        if (a.vout) a.vout[p] = vo;
}

template <bool kVar>
hipError_t launch_pass(DnArgs<kVar> a, hipStream_t s) {
    a.tiles_x = (a.w + 63) / 64;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.h + 3) / 4);
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles), block(64, 4);
    const bool z = a.sigma_z > 0.0f, l = a.sigma_l > 0.0f;
    if (z && l) hipLaunchKernelGGL((k_denoise_pass<true, true, kVar>), grid, block, 0, s, a);
    else if (z) hipLaunchKernelGGL((k_denoise_pass<true, false, kVar>), grid, block, 0, s, a);
    else if (l) hipLaunchKernelGGL((k_denoise_pass<false, true, kVar>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_denoise_pass<false, false, kVar>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_denoise_keys(const float4* al, const uint32_t* id, uint2* keys, size_t n, hipStream_t s) {
    const size_t blocks = std::min<size_t>((n + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(k_denoise_keys, dim3((unsigned)blocks), dim3(256), 0, s, al, id, keys, n);
    return hipGetLastError();
}

hipError_t launch_denoise_pass(const DnPass& pass, hipStream_t s) { return launch_pass<false>(pass, s); }
hipError_t launch_denoise_var_pass(const DnVarPass& pass, hipStream_t s) { return launch_pass<true>(pass, s); }

}  // namespace mm
