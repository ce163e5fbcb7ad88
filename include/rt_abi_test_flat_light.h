/* rt_abi_test_flat_light.h — the lab's probes of the area lights, beside include/rt_abi_test.h: exported by
 * librt_hip_probe.so only, never by a product library.  All pointers but the scene are DEVICE pointers; both calls enqueue on `stream`. */
#pragma once
#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The device form of the aim, one activation per thread: activation i = {pixel, sample, node of the hit} (d_pixel_sample_node, n x 3 u32)
 * shoots light d_j[i] of the scene's light list with the scene's seed — the light list, the entry's RESIDENT record and shape, child_node, the
 * draw at slot 0xFFFFFFFF, rt_flat_light_aim: what the flat arm of the lit QUADS megakernels runs — and d_T[i] (n x 3 f64) is the point aimed
 * at.  A d_j[i] that is not an emitter (a Light sphere, or past the list) gives three NaNs.  d_P (n x 3 f64, may be NULL) is where the light
 * rays start; T does not depend on it.  Launched with 192 threads a workgroup.  RT_ERR_INVALID: a null argument, a scene without an emitter. */
int rt_hip_flat_light_probe(RtHipScene*, const double* d_P, const uint32_t* d_pixel_sample_node, const uint32_t* d_j, double* d_T, uint32_t n, void* stream);
/* rt_flat_light_aim (csrc/common/rt_flat_light.h) compiled for the device, activation i on its own entry d_quv[i] (q, u, v: n x 9 f64), shape
 * d_triangle[i] (i32, non-zero: a triangle) and four words d_words[i] (n x 4 u32) -> d_T (n x 3 f64): crafted words reach device code.
 * block: the workgroup size of the launch, 1 .. 1024. */
int rt_hip_flat_light_aim_probe(const double* d_quv, const int32_t* d_triangle, const uint32_t* d_words, double* d_T, uint32_t n, uint32_t block, void* stream);

#ifdef __cplusplus
}
#endif
