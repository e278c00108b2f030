// mm_temporal.h — the reprojection mm_accumulate_frames and mm_accumulate_frames_var share
// (include/mm_api.h states the arithmetic): the rotation, the projection of a pixel's virtual image into
// the history frame's camera, a tap's address and the key test that confirms or refutes it.  Device code,
// included by temporal_kernels.hip: the plain and the variance instances run the same operations.
#pragma once
#include <hip/hip_runtime.h>

#include "mm_launch.h"
#include "mm_trace.h"

namespace mm {

namespace {

// The rotation primary_dir applies to its normalised direction (mm_device.h), with the quaternion as arguments.
__device__ __forceinline__ F3 tp_rot(F3 q, float qw, F3 v) {
    const F3 nq = F3{-q.x, -q.y, -q.z};
    const float s1 = -dot3(nq, v);
    const F3 c1 = F3{nq.y * v.z - nq.z * v.y, nq.z * v.x - nq.x * v.z, nq.x * v.y - nq.y * v.x};
    const F3 v1 = c1 + qw * v;
    const F3 c2 = F3{v1.y * q.z - v1.z * q.y, v1.z * q.x - v1.x * q.z, v1.x * q.y - v1.y * q.x};
    return (qw * v1 + s1 * q) + c2;
}

// Pixel (i, j)'s virtual image (dist along its mirror chain) in the history frame's window: false for NOHIST
// (behind the history camera, or outside [-1, w) x [-1, h)); else (uu, vv) and dp, the distance from that camera.
__device__ __forceinline__ bool tp_project(const TpFrame& a, uint32_t i, uint32_t j, float dist, float& uu, float& vv,
                                           float& dp) {
    mm_uniform u;
    u.cam = a.cam;
    u.view_w = a.view_w;
    u.view_h = a.view_h;
    const F3 d = primary_dir(u, a.x0 + i, a.y0 + j);
    const F3 X = F3{a.cam.center[0], a.cam.center[1], a.cam.center[2]} + dist * d;
    const F3 r = X - F3{a.h_cam.center[0], a.h_cam.center[1], a.h_cam.center[2]};
    const F3 l = tp_rot(F3{-a.h_cam.quat[0], -a.h_cam.quat[1], -a.h_cam.quat[2]}, a.h_cam.quat[3], r);
    dp = sqrtf(dot3(r, r));
    if (!(l.z > 0.0f)) return false;
    const float vx = a.h_cam.viewport[0], vy = a.h_cam.viewport[1];
    const float sx = ((((l.x * a.h_cam.focal) / l.z) + vx * 0.5f) * a.view_w) / vx;
    const float sy = ((((l.y * a.h_cam.focal) / l.z) + vy * 0.5f) * a.view_h) / vy;
    uu = sx - (float)a.x0;
    vv = sy - (float)a.y0;
    return uu >= -1.0f && uu < (float)a.w && vv >= -1.0f && vv < (float)a.h;
}

// Tap (qx, qy) of the history frame: whether it lies in the tile, and its address clamped into the frame
// (always a pixel of the history frame: cy * w + cx < w * h < 2^31).
__device__ __forceinline__ uint32_t tp_tap(const TpFrame& a, int qx, int qy, bool& in) {
    in = (uint32_t)qx < a.w && (uint32_t)qy < a.h;
    const uint32_t cx = (uint32_t)min(max(qx, 0), (int)a.w - 1), cy = (uint32_t)min(max(qy, 0), (int)a.h - 1);
    return cy * a.w + cx;
}

// The key test of a tap inside the tile: id, mirror hits, normal and distance.
__device__ __forceinline__ bool tp_key(const TpFrame& a, bool in, uint32_t idq, uint32_t idp, float mhq, float mhp,
                                       const float4& ndp, const float4& ndq, float dp) {
    const float dn = (ndp.x * ndq.x + ndp.y * ndq.y) + ndp.z * ndq.z;
    bool take = in;
    take &= idq == idp;
    take &= mhq == mhp;
    take &= dn >= 0.0f;
    take &= fabsf(dp - ndq.w) <= a.tol_z * (dp + ndq.w);
    return take;
}

}  // namespace

}  // namespace mm
