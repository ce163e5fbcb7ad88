/* rt_abi_test_flat_motion.h — the lab's probe of the device surface of flat primitives that move within the frame,
 * beside include/rt_abi_test.h: exported by librt_hip_probe.so only, never by a product library.  All pointers but the scene are DEVICE
 * pointers; the call enqueues on `stream`. */
#pragma once
#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a QUADS ∧ MOTION megakernel does for a segment, one ray per thread, without the megakernel around it: ray i = d_rays[i] (n x 6 f64:
 * origin, direction) at shutter time d_tau[i] (n f32; NULL: 0) with the closest-so-far d_closest[i] (n f64) and the hit it already holds,
 * d_best_in[i] (n i32; NULL: -1; any int: an id below the scene's sphere count is "a sphere") — the motion tables at tau, flats_hit through
 * them (the scan, the structure or the moving walk, chosen behind the scene's own bits) — and d_best[i] (n i32) is the id it returns, always
 * written.  Where that id is a flat entry and not the d_best_in[i] that came in, object_surface<true> runs on it — in a scene with shading
 * normals or motion records the cold flat_surface_shutter — and d_t[i], d_point[i], d_normal[i] (n x 3 f64), d_front[i] (n i32) and
 * d_origin[i] (n x 3 f64: the entry's origin at tau, the frame of a solid pattern and of the image lookup) are written; every other ray
 * leaves them as they were.  block: the workgroup size of the launch, 1 .. 1024; n = 0 launches nothing.
 * RT_ERR_INVALID: a null argument other than d_tau and d_best_in, a block out of range, a scene without flat primitives, a scene in which
 * nothing moves within the frame (it selects no MOTION kernel). */
int rt_hip_flat_shutter_probe(RtHipScene*, const double* d_rays, const float* d_tau, const double* d_closest, const int32_t* d_best_in,
                              uint32_t n, uint32_t block,
                              int32_t* d_best, double* d_t, double* d_point, double* d_normal, int32_t* d_front, double* d_origin, void* stream);

#ifdef __cplusplus
}
#endif
