// mm_denoise.h — the pieces of the a-trous pass kernel (denoise_kernels.hip: mm_denoise_frames and, as its kVar
// instances, mm_denoise_frames_var): the luminance, the packed key read, the three-clause surface test and the
// guarded quotient with its range tests.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "mm_trace.h"

namespace mm {

__device__ __forceinline__ float dn_lum(const float4& c) { return (0.25f * c.x + 0.5f * c.y) + 0.25f * c.z; }

// The key of pixel i: (id, al.w).  Two keys are equal when the ids are (all 32 bits) and the al.w are as floats.
// (Pass: DnPass or DnVarPass, mm_launch.h -- its `keys`.)
template <typename Pass>
__device__ __forceinline__ void dn_key(const Pass& a, uint32_t i, uint32_t& id, float& mh) {
    const uint2 k = a.keys[i];
    id = k.x;
    mh = __uint_as_float(k.y);
}

// RN(a / d) without the compiler's IEEE division sequence: Markstein's quotient over y = RN(1/d) (mm_trace.h
// qdiv, rcp_guarded: 6 operations instead of ~12).  It is the correctly rounded quotient when nothing under- or
// overflows on the way.  The conditions used here, with room to spare:
//   dn_den_ok  |d| in [2^-40, 2^40]          (rcp_guarded's verified range is [2^-44, 2^44]);
//   dn_num_ok  a = 0 or |a| in [2^-60, 2^60];
// then |a / d| lies in [2^-100, 2^100] and the exact residual a - q*d, whose lowest bit is above 2^-48 |a|, is a
// normal float.  A NaN fails either test.  A zero numerator gives a zero (its sign may differ from IEEE's; both
// quotients t below are used as t * t only) or, over a denominator whose reciprocal is not finite, a NaN, which
// the test of 1 + t*t then catches.  The weights g need no test: they start as 2^-8 .. 9/64 and are divided at
// most twice by an f in [1, 2^40].
__device__ __forceinline__ bool dn_den_ok(float d) {
    bool ok = fabsf(d) >= 0x1p-40f;
    ok &= fabsf(d) <= 0x1p40f;
    return ok;
}
__device__ __forceinline__ bool dn_num_ok(float a) {
    bool ok = fabsf(a) >= 0x1p-60f;
    ok &= fabsf(a) <= 0x1p60f;
    ok |= a == 0.0f;
    return ok;
}
__device__ __forceinline__ float dn_div(float a, float d) { return qdiv(a, d, rcp_guarded(d)); }

struct DnPixel {
    float4 C, nd;   // the centre's colour and (normal, distance)
    uint32_t id;    // its key
    float mh;
    float lum;
    uint32_t x, y;  // in the frame (w * h < 2^31: mm_denoise_frames)
};

// Whether tap q shows the centre's surface (the three-clause test of the specification).
template <typename Pass>
__device__ __forceinline__ bool dn_same_surface(const Pass& a, const DnPixel& c, uint32_t q, const float4& ndq) {
    uint32_t idq;
    float mhq;
    dn_key(a, q, idq, mhq);
    const float d = (c.nd.x * ndq.x + c.nd.y * ndq.y) + c.nd.z * ndq.z;
    bool same = idq == c.id;
    same &= mhq == c.mh;
    same &= d >= 0.0f;
    return same;
}

}  // namespace mm
