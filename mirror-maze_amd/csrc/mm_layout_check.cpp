// mm_layout_check.cpp — compile-time proof that the C ABI structs are
// byte-identical to the reference's #[repr(C)] types / Metal structs.
#include <cstddef>

#include "mm_types.h"

// Plane (src/main.rs:51-58) / rect (src/shaders.metal:19-24): 4 x packed_float3
static_assert(sizeof(mm_rect) == 48, "Plane is 48 B");
static_assert(offsetof(mm_rect, v) == 12 && offsetof(mm_rect, u) == 24 && offsetof(mm_rect, color) == 36,
              "Plane field offsets");
// BVHNode (src/main.rs:74-81) / bvh_node (src/shaders.metal:30-35)
static_assert(sizeof(mm_node) == 32, "BVHNode is 32 B");
static_assert(offsetof(mm_node, mx) == 12 && offsetof(mm_node, left_first) == 24 && offsetof(mm_node, count) == 28,
              "BVHNode field offsets");
// Camera (src/main.rs:32-39) / camera (src/shaders.metal:37-42)
static_assert(sizeof(mm_camera) == 40, "Camera is 40 B");
static_assert(offsetof(mm_camera, focal) == 12 && offsetof(mm_camera, quat) == 16 && offsetof(mm_camera, viewport) == 32,
              "Camera field offsets");
// Uniform (src/main.rs:41-49) / uni (src/shaders.metal:237-243)
static_assert(sizeof(mm_uniform) == 56, "Uniform is 56 B");
static_assert(offsetof(mm_uniform, view_w) == 40 && offsetof(mm_uniform, view_h) == 44 &&
                  offsetof(mm_uniform, chunk_w) == 48 && offsetof(mm_uniform, time) == 52,
              "Uniform field offsets");
static_assert(sizeof(mm_ext) == 24, "mm_ext is 24 B");
static_assert(sizeof(mm_stats) == 32, "mm_stats is 32 B");
static_assert(sizeof(mm_aov) == 24 && offsetof(mm_aov, albedo) == 8 && offsetof(mm_aov, id) == 16,
              "mm_aov is three pointers");
static_assert(sizeof(mm_denoise_params) == 16 && offsetof(mm_denoise_params, sigma_z) == 4 &&
                  offsetof(mm_denoise_params, flags) == 12,
              "mm_denoise_params is four 4-byte fields");
static_assert(sizeof(mm_denoise_var_params) == 24 && offsetof(mm_denoise_var_params, sigma_z) == 4 &&
                  offsetof(mm_denoise_var_params, sigma_l) == 8 && offsetof(mm_denoise_var_params, eps_l) == 12 &&
                  offsetof(mm_denoise_var_params, flags) == 16 && offsetof(mm_denoise_var_params, reserved) == 20,
              "mm_denoise_var_params is six 4-byte fields");
static_assert(sizeof(mm_temporal_params) == 16 && offsetof(mm_temporal_params, tol_z) == 4 &&
                  offsetof(mm_temporal_params, w_min) == 8 && offsetof(mm_temporal_params, flags) == 12,
              "mm_temporal_params is four 4-byte fields");
static_assert(sizeof(mm_temporal_prev) == 72 && offsetof(mm_temporal_prev, guides) == 8 &&
                  offsetof(mm_temporal_prev, cam) == 32,
              "mm_temporal_prev is a pointer, an mm_aov and an mm_camera");
static_assert(sizeof(mm_temporal_prev_var) == 80 && offsetof(mm_temporal_prev_var, guides) == 8 &&
                  offsetof(mm_temporal_prev_var, cam) == 32 && offsetof(mm_temporal_prev_var, var) == 72,
              "mm_temporal_prev_var is mm_temporal_prev and a pointer");
static_assert(sizeof(mm_upsample_params) == 16 && offsetof(mm_upsample_params, w_min) == 4 &&
                  offsetof(mm_upsample_params, flags) == 8 && offsetof(mm_upsample_params, reserved) == 12,
              "mm_upsample_params is four 4-byte fields");

extern "C" int mm_layout_ok(void) { return 1; }
