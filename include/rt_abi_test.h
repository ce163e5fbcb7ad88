/*
 * rt_abi_test.h — device probes and diagnostics of the MI355X path tracer: TEST INFRASTRUCTURE, not part of the seam.
 *
 * These entry points exist in librt_hip_probe.so only (the same sources as librt_hip.so compiled with -DRT_TEST_PROBES;
 * rust-raytracer_amd/build.py) — the product library exports none of them.  tests/test_gpu_parity.py, tests/test_walk_rays_gpu.py,
 * tests/test_quad_rays_gpu.py, tests/test_medium_rays_gpu.py, tests/test_solid_points_gpu.py and tools/diag.py bind them; a host that replaces raytracer.rs:260-262 needs include/rt_abi.h alone.
 */
#ifndef RT_ABI_TEST_H
#define RT_ABI_TEST_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics (builds with -DRT_PROFILE only; other builds return stale memory): the 32 raw
 * launch counters, then {start, end, time the
 * wave found the tile queue empty, iterations after that | lanes x iterations << 32} of every
 * wave of the last launch, on the chip-wide 100 MHz clock.  Returns the number of waves copied
 * (out holds 32 + 4 x max_waves uint64) or a negative RtStatus. */
int rt_hip_debug_timeline(RtHipScene*, uint64_t* out, uint32_t max_waves);
/* Diagnostics: the deepest camera path per pixel tile that the last MEASURING frame recorded (tile_order 2: the first two
 * frames of a view) — what the queue order of later frames is sorted by.  out[tile], row-major over the launch's tile grid
 * (*tiles_x tiles wide); returns the number of tiles copied (<= cap) or a negative RtStatus. */
int rt_hip_debug_tile_depth(RtHipScene*, uint32_t* out, uint32_t cap, uint32_t* tiles_x);
/* Device self-tests (device pointers; tests/test_gpu_parity.py): correctly rounded f64 sqrt / divide,
 * f32 sqrt and atan2 of n operands; Sphere::hit (sphere.rs:46-58) of n (ray, sphere) pairs through
 * the kernel's own hit test — rays = n x {origin[3], direction[3]}, spheres = n x {center[3], radius},
 * out_t = the accepted root with t_max = f64::MAX, or -1. */
int rt_hip_math_probe(const double* x, const double* y, double* out_sqrt, double* out_div, float* out_sqrtf, double* out_atan2,
                      uint32_t n, void* stream);
int rt_hip_hit_probe(const double* rays, const double* spheres, double* out_t, uint32_t n, void* stream);
/* f64::atan2 (sphere.rs:39) of n (y, x) pairs through the device build of the routine kernel and CPU checker share
 * (csrc/common/rt_atan2.h): tests compare it with a committed fixture of correctly rounded results. */
int rt_hip_atan2_probe(const double* d_y, const double* d_x, double* d_out, uint32_t n, void* stream);
/* The texel of a Texture hit on the device, both ways (materials.rs:236-254 through sphere.rs:35-43): the kernel's fast
 * (u, v) — v_rsq_f64 / v_rcp_f64 + Newton steps, which only the device build takes — beside the exact path, for n hit
 * points (device, 3 doubles each) on the sphere centre_radius (host, 4 doubles).  d_out = n x {fast_ok, fast col, fast
 * row, exact col, exact row} (u64); d_uv (optional) = n x {fast u, fast v, exact u, exact v}, fast u = NaN where the fast
 * path declined.  rt_hip_quot_probe: rt_fast_quot(x, y), rt_fast_rsqrt(x) and (d_div optional) rt_div_inrange(x, y) — the
 * library division without range scaling and fix-up: must equal the IEEE quotient — of n positive normal operands. */
int rt_hip_texel_probe(const double* d_points, const double centre_radius[4], double h_offset, uint64_t tex_w, uint64_t tex_h,
                       uint64_t* d_out, double* d_uv, uint32_t n, void* stream);
int rt_hip_quot_probe(const double* d_x, const double* d_y, double* d_quot, double* d_rsqrt, double* d_div, uint32_t n, void* stream);
/* The grid walk on the device (tests/test_walk_rays_gpu.py).  rt_hip_render_rays_probe: one whole frame through the scene's
 * normal launch path (same instantiation, tiles and queue) in which every sample of pixel p starts from the camera ray
 * d_rays[6p .. 6p+5] = {origin[3], direction[3]} instead of the jittered one; its bounces follow Philox as usual.  Sample 0's
 * camera segment of pixel p writes the (t, sphere) hit_world returned to d_first_t[p] / d_first_sphere[p] (both or neither;
 * -1: no hit).  Waits for the frame and fills stats; the scene's learned queue order is neither measured nor changed.
 * rt_hip_walk_probe: rt_core.h hit_world_grid — the per-lane walk tests/hostsim runs — of n rays {origin[3], direction[3]}
 * through the scene's tables, one per thread; d_t / d_best = its (t, sphere), t = f64::MAX and sphere = -1 without a hit;
 * d_work (optional) = n x {exact sphere tests, grid steps} of each walk.
 * All d_* are device pointers; rays of d_rays are pixel-major over the scene's width x height. */
int rt_hip_render_rays_probe(RtHipScene*, const double* d_rays, double* d_first_t, int32_t* d_first_sphere, void* d_rgb8, void* d_linear,
                             RtStats* stats);
int rt_hip_walk_probe(RtHipScene*, const double* d_rays, double* d_t, int32_t* d_best, uint32_t* d_work, uint32_t n, void* stream);
/* The quad code on the device (tests/test_quad_rays_gpu.py): rt_core.h quads_hit — the QUADS arm of hit_world — of n rays
 * d_rays[6i .. 6i+5] = {origin[3], direction[3]}, one per thread, against the scene's quads first_quad .. first_quad + n_quads - 1 in that
 * order, each ray with its own closest hit so far d_closest[i] and no earlier object; on a hit, object_surface<true> of the accepted id.
 * d_best[i] = the id (n_spheres + k) or -1; on a hit d_t[i], d_point[3i..], d_normal[3i..] (the hit normal) and d_front[i] (front_face,
 * 0 / 1) are written, on a miss they are left as they were.  A range outside the scene's quads is RT_ERR_INVALID.  Any double is a valid
 * component of a ray or a closest: the quad test is arithmetic alone.  All d_* are device pointers. */
int rt_hip_quad_probe(RtHipScene*, const double* d_rays, const double* d_closest, uint32_t n, uint32_t first_quad, uint32_t n_quads,
                      int32_t* d_best, double* d_t, double* d_point, double* d_normal, int32_t* d_front, void* stream);
/* The media and solid-texture code on the device (tests/test_medium_rays_gpu.py, tests/test_solid_points_gpu.py).  Their
 * contract is the bits of csrc/common/rt_neg_log.h and csrc/common/rt_solid.h: every output below must equal the host build of the same
 * headers (tests/lanesim) bit for bit.  All d_* are device pointers; n = 0 is allowed and launches nothing.
 * rt_hip_neg_log_probe: rt_neg_log of n doubles.  Any double is a valid argument (0 -> +inf, negative and NaN -> NaN, +inf -> -inf).
 * rt_hip_solid_fn_probe: rt_solid_noise(p, seed) -> d_noise[i], rt_solid_noise_factor(p, mode, octaves, seed) -> d_factor[i] and
 * rt_solid_checker_odd(p) -> d_checker_odd[i] (0 / 1) of the n points d_p[3i .. 3i+2], which are already in the sphere's frame and scaled;
 * each of the three outputs may be null.  Any double is a valid coordinate.  mode 0..2 (noise, turbulence, marble) and octaves 1..16, else
 * RT_ERR_INVALID.
 * rt_hip_solid_probe: rt_core.h solid_albedo — the colour a hit attenuates by — of the n world-space points d_points[3i .. 3i+2] on sphere
 * `sphere` of the scene, with that sphere's own centre and material record: d_rgb[3i .. 3i+2] (f32).  A sphere that is neither Checker nor
 * Noise, or an index >= the scene's spheres, is RT_ERR_INVALID.
 * rt_hip_medium_probe: hit_world as a MEDIUM kernel runs it for one segment — hit_world_grid with the medium candidate, then the flat
 * primitives of a scene that has some — of n rays d_rays[6i .. 6i+5] = {origin[3], direction[3]}, one per thread.  Ray i has the RNG address
 * (pixel i, sample 0, node d_node[i], the scene's seed) and is taken at shutter time d_tau[i] (f32; null: 0; read only by a scene that
 * moves).  d_t / d_best = its (t, object id); a miss leaves t = f64::MAX and best = -1.  d_work (optional) = n x {exact sphere tests, grid
 * steps}.  A scene without media is RT_ERR_INVALID.  Any double is a valid component of a ray. */
int rt_hip_neg_log_probe(const double* d_x, double* d_out, uint32_t n, void* stream);
int rt_hip_solid_fn_probe(const double* d_p, uint32_t mode, uint32_t octaves, uint32_t seed, double* d_noise, double* d_factor, int32_t* d_checker_odd,
                          uint32_t n, void* stream);
int rt_hip_solid_probe(RtHipScene*, uint32_t sphere, const double* d_points, float* d_rgb, uint32_t n, void* stream);
int rt_hip_medium_probe(RtHipScene*, const double* d_rays, const float* d_tau, const uint32_t* d_node, double* d_t, int32_t* d_best, uint32_t* d_work,
                        uint32_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_TEST_H */
