/*
 * rt_oracle.h — CPU oracle of the ray_color hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product (librt_hip.so, librt_host.so, the
 * `raytracer` CLI, the python package) may link, load or call this library.  Its only users
 * are tests/, __graft_entry__.smoke() and bench.py's `cpu_baseline` leg.
 *
 * It restates, in plain C with f64 geometry / f32 colour and NO fused multiply-adds
 * (-ffp-contract=off, like rustc), the reference functions
 *   raytracer/src/raytracer.rs:44-59  hit_world      :61-69  clamp      :71-165 ray_color
 *   raytracer/src/raytracer.rs:191-218 render_line   :220-229 find_lights :250-266 render
 *   raytracer/src/sphere.rs:35-79     u_v_from_sphere_hit_point, Sphere::hit
 *   raytracer/src/materials.rs:44-54, 65-69, 84-95, 111-129, 144-155, 176-199, 236-267
 *   raytracer/src/camera.rs:45-84     Camera::new, get_ray
 *   raytracer/src/point3d.rs:22-38, 52-177
 * with one substitution: rand::thread_rng() (OS-seeded ChaCha, unreproducible) is replaced
 * by counter-based Philox4x32-10 addressed by (pixel, sample, path node, slot); see
 * DESIGN.md "RNG addressing".
 *
 * Parity pinning: the reference cannot be built here (no cargo/rustc), it holds no golden
 * images and its RNG is unseeded, so IMAGE parity against the Rust binary is unpinned by
 * construction.  What IS pinned: every known-answer unit test the reference holds for this
 * path is replayed against the functions below in tests/test_oracle_kat.py,
 * and the Philox core is pinned by the Random123 known-answer vectors.
 */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H

#include "../include/rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* render() minus PNG: raytracer.rs:250-263.  rgb8 and linear are host buffers of
 * rt_tiles_local_rows()*width*3 bytes / floats (either may be NULL).  n_threads<=0 -> all
 * cores (one scanline per task, dynamic schedule = rayon's work stealing). */
int rt_oracle_render(const RtScene* scene, const RtRowTiles* tiles, uint8_t* rgb8, float* linear,
                     RtStats* stats, int n_threads);
/* the same for pixels [x0, x1) of those rows only (buffers still hold whole rows; other pixels are left untouched) */
int rt_oracle_render_window(const RtScene* scene, const RtRowTiles* tiles, uint32_t x0, uint32_t x1, uint8_t* rgb8,
                            float* linear, RtStats* stats, int n_threads);
/* Progressive rendering restated from include/rt_abi.h: samples [sample_begin, sample_begin + sample_count) of pixels [x0, x1) of
 * the selected rows (render_line's camera jitter, get_ray and ray_color with the RNG at sample index s), each ADDED to `accum`
 * (rt_tiles_local_rows()*width*3 u64, packed like rgb8) by the ABI's rule: a NaN channel sets bit 63, any other value is
 * clamped to [0, 1] and floor(v * 2^40 + 0.5) is added.  Other words are left untouched.  stats: as rt_oracle_render's. */
int rt_oracle_accumulate(const RtScene* scene, const RtRowTiles* tiles, uint32_t x0, uint32_t x1, uint32_t sample_begin,
                         uint32_t sample_count, uint64_t* accum, RtStats* stats, int n_threads);
/* rt_oracle_render (whole frame) with the camera ray of every sample of pixel p = y * width + x taken from rays[6p .. 6p+5] =
 * {origin[3], direction[3]} instead of get_ray's; the jitter's RNG words, the rest of each path and the statistics are as
 * rt_oracle_render's.  The device side is rt_hip_render_rays_probe (include/rt_abi_test.h). */
int rt_oracle_render_rays(const RtScene* scene, const double* rays, uint8_t* rgb8, float* linear, RtStats* stats, int n_threads);
int rt_oracle_threads(void);

/* ---- the extensions of the schema: thin lens and motion blur ----
 * Restated from the contract (include/rt_abi.h), not from the kernel:
 *   shutter time   tau = (philox(pixel, s, 0xFFFFFFFD, 0).x >> 8) * 2^-24, one per sample, used by every segment of the sample,
 *                  nested light rays included;
 *   moving sphere  dv = center1 - center (one f64 subtraction per component, a zero component stored as -0.0); its centre at tau is
 *                  c0 + dv * tau (a product and a sum, each rounded); Sphere::hit, the normal (p - c) / r and the texture's (u, v) from
 *                  p - c use that centre; light rays aim at the static light centres;
 *   lens           the jitter stays at node 0xFFFFFFFF slot 0; the lens point comes from attempts a = 0, 1, ... of
 *                  W = philox(pixel, s, 0xFFFFFFFF, 1 + a): candidates (range_m1_1(W.x), range_m1_1(W.y)) then (W.z, W.w), the first with
 *                  px*px + py*py < 1; offset = u*(r*px) + v*(r*py); the ray starts at origin + offset with direction
 *                  (((lower_left + horizontal*u_s) + vertical*v_s) - origin) - offset, the scene's camera vectors being
 *                  rt_camera_derive_lens's (on the focus plane).
 * Every member is optional.  ext NULL, center1 NULL or equal to every centre, and lens_r 0 give the plain entry points' results bit
 * for bit, statistics included.  RT_ERR_INVALID (as rt_hip_scene_create_moving / rt_hip_set_lens refuse them): a center1 - center
 * that is not finite, a Light sphere that moves, a lens_r that is negative or not finite, lens_r != 0 without lens_u and lens_v. */
typedef struct RtOracleExt {
  const double* center1; /* n_spheres x 3: the centres at shutter close; NULL = static */
  const double* lens_u;  /* rt_hip_set_lens's arguments: the camera's unit vectors u and v ... */
  const double* lens_v;
  double lens_r;         /* ... and the lens radius aperture / 2; 0 = the pinhole */
} RtOracleExt;
/* rt_oracle_render_window / rt_oracle_accumulate through the extension */
int rt_oracle_render_window_ext(const RtScene* scene, const RtRowTiles* tiles, uint32_t x0, uint32_t x1, const RtOracleExt* ext,
                                uint8_t* rgb8, float* linear, RtStats* stats, int n_threads);
int rt_oracle_accumulate_ext(const RtScene* scene, const RtRowTiles* tiles, uint32_t x0, uint32_t x1, uint32_t sample_begin,
                             uint32_t sample_count, const RtOracleExt* ext, uint64_t* accum, RtStats* stats, int n_threads);
/* hook: the camera ray and the shutter time of sample s of pixel (x, y): out = origin[3], direction[3], tau (tau is the contract's
 * draw whether or not a sphere moves) */
int rt_oracle_camera_ray_ext(const RtScene* scene, const RtOracleExt* ext, uint32_t x, uint32_t y, uint32_t s, double out[7]);

/* ---- hooks for the reference's known-answer tests ---- */
/* Philox4x32-10, Random123 layout */
void rt_oracle_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* sphere.rs:46-78; returns 1 on hit. out = t, p[3], normal[3], front_face, u, v (10 doubles) */
int rt_oracle_sphere_hit(const double center[3], double radius, const double origin[3],
                         const double dir[3], double t_min, double t_max, double out[10]);
/* f64::atan2 of sphere.rs:39 as both sides evaluate it (rust-raytracer_amd/csrc/common/rt_atan2.h) */
double rt_oracle_atan2(double y, double x);
void rt_oracle_atan2_v(const double* y, const double* x, double* out, uint64_t n); /* ... of n pairs */
/* point3d.rs:52-177 one operation at a time: op 0 add, 1 sub, 2 neg, 3 mul (componentwise), 4 div (componentwise),
 * 5 mul by s, 6 div by s, 7 dot -> out[0], 8 length_squared -> out[0], 9 near_zero -> out[0], 10 length -> out[0],
 * 11 unit_vector, 12 cross; returns -1 for an unknown op */
int rt_oracle_p3_op(int op, const double a[3], const double b[3], double s, double out[3]);
/* ray.rs:18-20 Ray::at */
void rt_oracle_ray_at(const double origin[3], const double dir[3], double t, double out[3]);
/* materials.rs:144-149 */
void rt_oracle_refract(const double uv[3], const double n[3], double etai_over_etat, double out[3]);
/* materials.rs:151-155 */
double rt_oracle_reflectance(double cosine, double ref_idx);
/* materials.rs:111-113 */
void rt_oracle_reflect(const double v[3], const double n[3], double out[3]);
/* camera.rs:45-77; out = origin, lower_left, horizontal, vertical, focal_length (13 doubles) */
void rt_oracle_camera_new(const double look_from[3], const double look_at[3], const double vup[3],
                          double vfov_deg, double aspect, double out[13]);
/* camera.rs:79-84; out = origin[3], direction[3] */
void rt_oracle_get_ray(const RtScene* scene, double u, double v, double out[6]);
/* raytracer.rs:71-165 for one explicit ray at (pixel,sample) RNG address; root call */
void rt_oracle_ray_color(const RtScene* scene, const double origin[3], const double dir[3],
                         uint32_t max_depth, uint32_t depth, uint32_t pixel, uint32_t sample,
                         float out_rgb[3]);
/* materials.rs:236-254 Texture::get_albedo */
void rt_oracle_texture_albedo(const RtSphere* s, const RtTexture* tex, double u, double v,
                              float out_rgb[3]);
/* raytracer.rs:213: palette f32 -> u8 */
uint8_t rt_oracle_f32_to_u8(float x);
/* raytracer.rs:220-229 */
uint32_t rt_oracle_find_lights(const RtSphere* spheres, uint32_t n, uint32_t* out_idx, uint32_t cap);
/* the two RNG draw flavours: (53-bit gen::<f64>(), gen_range(-1..1) grid) for a counter */
void rt_oracle_draws(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t node, uint32_t slot,
                     double out_u01[2], double out_range[3]);

#ifdef __cplusplus
}
#endif
#endif
