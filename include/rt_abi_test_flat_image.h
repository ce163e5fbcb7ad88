/* rt_abi_test_flat_image.h — the lab's probes of the images on flat primitives, beside include/rt_abi_test.h: exported by
 * librt_hip_probe.so only, never by a product library.  All pointers but the scene are DEVICE pointers; both calls enqueue on `stream`. */
#pragma once
#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the arm in lane_shade runs, one hit per thread: hit i lies at d_P[i] (n x 3 f64) on entry d_k[i] of the scene, whose origin at the
 * sample's shutter time is d_origin[i] (n x 3 f64) — the header slot in front of the records, the entry's resident image record and frame,
 * the fetch from the resident texels: the cold flat_image_albedo — and d_rgb[i] (n x 3 f32) is the attenuation.  An entry without an image
 * gives (-1, 0, 0); a d_k[i] outside the scene's entries gives three NaNs.  Launched with 192 threads a workgroup.
 * RT_ERR_INVALID: a null argument, a scene without an image. */
int rt_hip_flat_image_probe(RtHipScene*, const uint32_t* d_k, const double* d_origin, const double* d_P, float* d_rgb, uint32_t n, void* stream);
/* rt_flat_image_texel (csrc/common/rt_flat_image.h) compiled for the device, hit i on ITS OWN record d_rec[i] (n x 64 bytes: the resident
 * record {u32 texel_off, W, H, wrap; f64 uv[6]}, W > 0), frame d_ouvw[i] (O, u, v, w: n x 12 f64) and point d_P[i] (n x 3 f64) ->
 * d_texel[i] = {col, row, index} (n x 3 u32): crafted tables reach device code.  Nothing is fetched.
 * block: the workgroup size of the launch, 1 .. 1024. */
int rt_hip_flat_image_texel_probe(const void* d_rec, const double* d_ouvw, const double* d_P, uint32_t* d_texel, uint32_t n, uint32_t block, void* stream);

#ifdef __cplusplus
}
#endif
