// upsample_kernels.hip — mm_upsample_frames and mm_fill_pixels (include/mm_api.h states the arithmetic;
// tests/upsample_ref.c restates it in plain C and the GPU result equals it bit for bit).
//
//   k_upsample_frames  all frames of a call in one launch: one thread per output pixel, 64 x 4 blocks as
//                      k_temporal_frame and k_denoise_pass, so a wave is a 64-pixel row segment; the frame index
//                      is folded into the block index (block = frame * tiles + tile).  A pixel's four taps are
//                      the lattice pixels around it: 64 neighbouring lanes share 64 / scale + 1 lattice columns,
//                      and a block's four rows two or three lattice rows, so what reaches HBM is the pixel's
//                      own guides, its outputs and 1 / scale^2 of a lattice pixel (DESIGN.md §4 "Tracing a
//                      lattice and rebuilding from the AOVs").
//
// The taps are branch-free, as the temporal kernel's: addresses are clamped into the lattice, every load is
// unconditional and in bounds, and a tap outside the lattice, with no weight or refuted by the key test is
// computed and not added (a `take ? new : old` select, not a zero weight: the accumulators never see it).  The
// five divisions of a pixel are the compiler's correctly rounded sequences (the build's default).
//
//   kLds               MM_OPT_UPSAMPLE_LDS 1, the default: the block's lattice footprint (at most 33 x 3 pixels,
//                      3.9 KB) staged in LDS first, one load per footprint pixel instead of one per lane and
//                      tap; the same arithmetic on the same values.  0: direct gathers.  Staging measured 0.78
//                      (scale 2) and 0.87 (scale 4) of the gathers' time (profiles/upsample/ab.txt).
//   kVar / kWeight     instantiations of their own: the plain form loads no lattice variance and stores neither
//                      a variance nor a weight, and computes G2 only where a weight is stored.  kVar follows the
//                      variance OUTPUT: lattice variances given without one are not read.
//   k_fill_pixels      one lane per list entry, the twin of k_blend_pixels that replaces instead of blending;
//                      its optional images are uniform branches.
#include <hip/hip_runtime.h>

#include "mm_launch.h"
#include "mm_types.h"

namespace mm {

namespace {

// The lattice footprint of a 64 x 4 block: 64 / scale + 1 columns, and the rows its four pixel rows (4-aligned)
// reach, at most (scale 2) three.
constexpr uint32_t kUpStageMax = 33 * 3;

template <bool kVar, bool kWeight, bool kLds>
__global__ __launch_bounds__(256) void k_upsample_frames(const UpFrames a) {
    const uint32_t f = blockIdx.x / a.tiles, t = blockIdx.x - f * a.tiles;
    const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const uint32_t i = tx * 64 + threadIdx.x;  // (tiles_x * 64 < w + 64)
    const uint32_t j = ty * 4 + threadIdx.y;
    // (f * w * h + a pixel < 2^40: 64-bit element offsets; a frame's own offsets stay below 2^31)
    const size_t fo = (size_t)f * ((size_t)a.w * a.h), lo = (size_t)f * ((size_t)a.lw * a.lh);
    // kLds (MM_OPT_UPSAMPLE_LDS 1, the default): the block's lattice footprint staged once -- the same clamped,
    // in-bounds loads, one per footprint pixel instead of one per lane and tap -- and the taps read from LDS.
    __shared__ float4 s_low[kLds ? kUpStageMax : 1], s_nm[kLds ? kUpStageMax : 1];  // colour; (normal, mirror hits)
    __shared__ uint32_t s_id[kLds ? kUpStageMax : 1];
    __shared__ float s_var[kLds && kVar ? kUpStageMax : 1];
    const uint32_t Xb = (tx * 64) >> a.shift, Yb = (ty * 4) >> a.shift, cols = (64u >> a.shift) + 1;
    if constexpr (kLds) {
        const uint32_t rows = max(4u >> a.shift, 1u) + 1, e = threadIdx.y * 64 + threadIdx.x;
        if (e < cols * rows) {
            const uint32_t ey = e / cols, ex = e - ey * cols;
            const uint32_t cx = min(Xb + ex, a.lw - 1), cy = min(Yb + ey, a.lh - 1);
            const size_t q = fo + ((cy << a.shift) * a.w + (cx << a.shift));
            const size_t lq = lo + (cy * a.lw + cx);
            const float4 n = a.nd[q];
            s_low[e] = a.low[lq];
            s_nm[e] = make_float4(n.x, n.y, n.z, a.al[q].w);
            s_id[e] = a.id[q];
            if constexpr (kVar) s_var[e] = a.vlow[lq];
        }
        __syncthreads();
    }
    if (i >= a.w || j >= a.h) return;
    const size_t p = fo + (j * a.w + i);
    const uint32_t idp = a.id[p];
    const float4 ndp = a.nd[p];
    const float mhp = a.al[p].w;
    const uint32_t X0 = i >> a.shift, Y0 = j >> a.shift;
    const float fa = (float)(i - (X0 << a.shift)) * a.inv_s, fb = (float)(j - (Y0 << a.shift)) * a.inv_s;
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, W = 0.0f, G2 = 0.0f, SV = 0.0f;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
        const uint32_t dx = tap & 1, dy = tap >> 1;
        const uint32_t Qx = X0 + dx, Qy = Y0 + dy;
        const bool in = Qx < a.lw && Qy < a.lh;
        // clamped into the lattice: (lw - 1) * scale <= w - 1 and (lh - 1) * scale <= h - 1, so q is a pixel
        // of frame f and lq a lattice pixel of it
        const uint32_t cx = min(Qx, a.lw - 1), cy = min(Qy, a.lh - 1);
        float4 Lq, ndq;  // ndq.w: unused
        uint32_t idq;
        float mhq, Vq = 0.0f;
        if constexpr (kLds) {
            const uint32_t e = (Qy - Yb) * cols + (Qx - Xb);  // (inside the footprint: the entry of the clamped pixel)
            Lq = s_low[e];
            ndq = s_nm[e];
            mhq = ndq.w;
            idq = s_id[e];
            if constexpr (kVar) Vq = s_var[e];
        } else {
            const size_t q = fo + ((cy << a.shift) * a.w + (cx << a.shift));
            const size_t lq = lo + (cy * a.lw + cx);
            Lq = a.low[lq];
            idq = a.id[q];
            ndq = a.nd[q];
            mhq = a.al[q].w;
            if constexpr (kVar) Vq = a.vlow[lq];
        }
        const float g = (dx ? fa : 1.0f - fa) * (dy ? fb : 1.0f - fb);
        const float dn = (ndp.x * ndq.x + ndp.y * ndq.y) + ndp.z * ndq.z;
        bool take = in;
        take &= g > 0.0f;
        take &= idq == idp;
        take &= mhq == mhp;
        take &= dn >= 0.0f;
        const float nx = Sx + g * Lq.x, ny = Sy + g * Lq.y, nz = Sz + g * Lq.z, nw = W + g;
        Sx = take ? nx : Sx;
        Sy = take ? ny : Sy;
        Sz = take ? nz : Sz;
        W = take ? nw : W;
        if constexpr (kWeight) {
            const float n2 = G2 + g * g;
            G2 = take ? n2 : G2;
        }
        if constexpr (kVar) {
            const float nv = SV + (g * g) * Vq;
            SV = take ? nv : SV;
        }
    }
    const bool hole = idp == MM_AOV_ID_FAILED || !(W >= a.w_min);
    const float4 o = make_float4(Sx / W, Sy / W, Sz / W, 1.0f);
    a.out[p] = hole ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : o;
    if constexpr (kWeight) {
        const float wt = (W * W) / G2;
        a.wout[p] = hole ? 0.0f : wt;
    }
    if constexpr (kVar) {
        const float v = SV / (W * W);
        a.vout[p] = hole ? 0.0f : v;
    }
}

// mm_fill_pixels (include/mm_api.h): entry e replaces its pixel of the window's images; one lane per entry.  An
// entry outside the window touches nothing (p is computed only inside it: p < w * h < 2^31).
__global__ __launch_bounds__(256) void k_fill_pixels(const UpFill b) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b.n) return;
    const uint2 r = b.pixels[e];
    if (r.x < b.x0 || r.x - b.x0 >= b.w || r.y < b.y0 || r.y - b.y0 >= b.h) return;
    const uint32_t p = (r.y - b.y0) * b.w + (r.x - b.x0);
    b.image[p] = b.extra[e];
    if (b.var) b.var[p] = b.extra_vmean[e];
    if (b.weight) b.weight[p] = b.m;
}

}  // namespace

hipError_t launch_upsample_frames(const UpFrames& frames, hipStream_t s) {
    UpFrames a = frames;
    a.tiles_x = (a.w + 63) / 64;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.h + 3) / 4);
    const uint64_t blocks = tiles * a.n_frames;
    if (blocks == 0 || blocks >= (1ull << 26)) return hipErrorInvalidValue;
    a.tiles = (uint32_t)tiles;
    const dim3 grid((unsigned)blocks), block(64, 4);
    const bool var = a.vout != nullptr, weight = a.wout != nullptr;
#define MM_UP_LAUNCH(V, W)                                                                               \
    do {                                                                                                 \
        if (a.lds) hipLaunchKernelGGL((k_upsample_frames<V, W, true>), grid, block, 0, s, a);           \
        else hipLaunchKernelGGL((k_upsample_frames<V, W, false>), grid, block, 0, s, a);                \
    } while (0)
    if (var && weight) MM_UP_LAUNCH(true, true);
    else if (var) MM_UP_LAUNCH(true, false);
    else if (weight) MM_UP_LAUNCH(false, true);
    else MM_UP_LAUNCH(false, false);
#undef MM_UP_LAUNCH
    return hipGetLastError();
}

hipError_t launch_fill_pixels(const UpFill& fill, hipStream_t s) {
    const uint64_t blocks = (fill.n + 255) / 256;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fill_pixels, dim3((unsigned)blocks), dim3(256), 0, s, fill);
    return hipGetLastError();
}

}  // namespace mm
