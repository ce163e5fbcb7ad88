/*
 * rt_solid.h — the solid textures: ONE checker and ONE lattice noise for the kernel (rt_core.h solid_albedo) and for
 * every restatement of them (tests/solid_mini.py), so that Checker and Noise spheres are bit-identical everywhere.
 *
 * What is the contract is the BITS: every function below is a fixed sequence of IEEE f64 operations (+, -, *, floor, fabs and
 * comparisons; no fused operation, no contraction, no library call, no table in memory) and wrapping u32 / i64 integer operations, so a
 * restatement in any language with IEEE doubles reproduces it.  All of them are pure functions of their arguments.
 *
 * The point p handed to them is in the SPHERE'S FRAME, scaled: q = hit point - the centre the accepted hit test used (the centre at
 * the sample's shutter time for a moving sphere), p = q * scale per component (rt_solid_point).
 *
 * Checker (rt_solid_checker_odd): f_c = floor(p_c); any !(fabs(f_c) < 2^52) (NaN included): even.  Else parity
 *   ((int64)f_x + (int64)f_y + (int64)f_z) & 1: 0 even, 1 odd.
 *
 * Lattice noise N(p, seed) (rt_solid_noise): any !(fabs(p_c) < 2^31): 0.0.  Else, per component,
 *   fl_c = floor(p_c), i_c = (uint32)(int32)(int64)fl_c, t_c = p_c - fl_c, s_c = t_c * t_c * (3.0 - 2.0 * t_c);
 *   the corner (dx, dy, dz) in {0, 1}^3 has the hash, in u32 arithmetic that wraps,
 *     h = (i_x + dx) * 0x9E3779B1 ^ (i_y + dy) * 0x85EBCA77 ^ (i_z + dz) * 0xC2B2AE3D ^ seed
 *     h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16        (the murmur3 finaliser)
 *   and the value Perlin's 2002 gradient rule gives for g = h & 15 on the offset (x, y, z) = (t_x - dx, t_y - dy, t_z - dz)
 *   (dx as 0.0 or 1.0):  a = g < 8 ? x : y;  b = g < 4 ? y : ((g == 12 || g == 14) ? x : z);
 *     value = ((g & 1) ? -a : a) + ((g & 2) ? -b : b).
 *   The eight values are blended dx innermost, then dy, then dz, each blend lo + s * (hi - lo) with lo the corner at 0:
 *     x00 = v000 + s_x * (v100 - v000), x10 = v010 + s_x * (v110 - v010), x01 = v001 + s_x * (v101 - v001), x11 = v011 + s_x * (v111 - v011)
 *     y0 = x00 + s_y * (x10 - x00), y1 = x01 + s_y * (x11 - x01);  N = y0 + s_z * (y1 - y0)        (v<dx><dy><dz>)
 *   N is exactly 0 at every lattice point (t = 0: the only corner with weight 1 has the offset 0) and |N| <= 1.5 (each
 *   corner value is at most |x| + |y| + |z| of its offset, and the weighted sum of those is at most 3 * 0.5); values slightly above 1
 *   do occur, so the `noise` factor below is clamped.
 *
 * The factor of a Noise sphere (rt_solid_noise_factor), one f64 in [0, 1]:
 *   mode 0 "noise":       f = 0.5 * (1.0 + N(p)), then f < 0.0 -> 0.0, f > 1.0 -> 1.0.
 *   mode 1 "turbulence":  acc = 0.0, w = 1.0, r = p; `octaves` times: acc += w * N(r); w *= 0.5; r = r * 2.0 (all three on every pass);
 *                         T = fabs(acc); f = T < 1.0 ? T : 1.0.
 *   mode 2 "marble":      the same T; x = 0.15915494309189535 * (p_z + 10.0 * T); x not finite: f = 0.0; else s = x - floor(x),
 *                         m = 1.0 - fabs(2.0 * s - 1.0), f = m * m * (3.0 - 2.0 * m).
 * The attenuation of a Noise sphere is (float)(f * (double)albedo_c) per channel.
 *
 * Plain C; RT_SOLID_FN may be predefined (e.g. `__host__ __device__ inline`).
 */
#ifndef RT_SOLID_H
#define RT_SOLID_H

#include <stdint.h>

#ifndef RT_SOLID_FN
#define RT_SOLID_FN static inline
#endif

#define RT_SOLID_KX 0x9E3779B1u
#define RT_SOLID_KY 0x85EBCA77u
#define RT_SOLID_KZ 0xC2B2AE3Du
#define RT_SOLID_M1 0x85EBCA6Bu
#define RT_SOLID_M2 0xC2B2AE35u
#define RT_SOLID_MODE_NOISE 0u
#define RT_SOLID_MODE_TURBULENCE 1u
#define RT_SOLID_MODE_MARBLE 2u
#define RT_SOLID_MAX_OCTAVES 16u
#define RT_SOLID_INV_2PI 0.15915494309189535

RT_SOLID_FN int rt_solid_checker_odd(double px, double py, double pz) {
  const double fx = __builtin_floor(px), fy = __builtin_floor(py), fz = __builtin_floor(pz);
  const double lim = 4503599627370496.0; /* 2^52 */
  if (!(__builtin_fabs(fx) < lim) || !(__builtin_fabs(fy) < lim) || !(__builtin_fabs(fz) < lim)) return 0;
  return (int)(((int64_t)fx + (int64_t)fy + (int64_t)fz) & 1);
}

RT_SOLID_FN uint32_t rt_solid_hash(uint32_t ix, uint32_t iy, uint32_t iz, uint32_t seed) {
  uint32_t h = (ix * RT_SOLID_KX) ^ (iy * RT_SOLID_KY) ^ (iz * RT_SOLID_KZ) ^ seed;
  h ^= h >> 16; h *= RT_SOLID_M1; h ^= h >> 13; h *= RT_SOLID_M2; h ^= h >> 16;
  return h;
}

RT_SOLID_FN double rt_solid_grad(uint32_t h, double x, double y, double z) {
  const uint32_t g = h & 15u;
  const double a = g < 8u ? x : y;
  const double b = g < 4u ? y : ((g == 12u || g == 14u) ? x : z);
  return ((g & 1u) ? -a : a) + ((g & 2u) ? -b : b);
}

RT_SOLID_FN double rt_solid_noise(double px, double py, double pz, uint32_t seed) {
  const double lim = 2147483648.0; /* 2^31 */
  if (!(__builtin_fabs(px) < lim) || !(__builtin_fabs(py) < lim) || !(__builtin_fabs(pz) < lim)) return 0.0;
  const double flx = __builtin_floor(px), fly = __builtin_floor(py), flz = __builtin_floor(pz);
  const uint32_t ix = (uint32_t)(int32_t)(int64_t)flx, iy = (uint32_t)(int32_t)(int64_t)fly, iz = (uint32_t)(int32_t)(int64_t)flz;
  const double tx = px - flx, ty = py - fly, tz = pz - flz;
  const double sx = tx * tx * (3.0 - 2.0 * tx), sy = ty * ty * (3.0 - 2.0 * ty), sz = tz * tz * (3.0 - 2.0 * tz);
  double yv[2];
  for (uint32_t dz = 0; dz < 2u; ++dz) {
    double xv[2];
    for (uint32_t dy = 0; dy < 2u; ++dy) {
      const double lo = rt_solid_grad(rt_solid_hash(ix, iy + dy, iz + dz, seed), tx, ty - (double)dy, tz - (double)dz);
      const double hi = rt_solid_grad(rt_solid_hash(ix + 1u, iy + dy, iz + dz, seed), tx - 1.0, ty - (double)dy, tz - (double)dz);
      xv[dy] = lo + sx * (hi - lo);
    }
    yv[dz] = xv[0] + sy * (xv[1] - xv[0]);
  }
  return yv[0] + sz * (yv[1] - yv[0]);
}

RT_SOLID_FN double rt_solid_turbulence(double px, double py, double pz, uint32_t octaves, uint32_t seed) {
  double acc = 0.0, w = 1.0;
  for (uint32_t k = 0; k < octaves; ++k) {
    acc += w * rt_solid_noise(px, py, pz, seed);
    w *= 0.5;
    px = px * 2.0; py = py * 2.0; pz = pz * 2.0;
  }
  return __builtin_fabs(acc);
}

RT_SOLID_FN double rt_solid_noise_factor(double px, double py, double pz, uint32_t mode, uint32_t octaves, uint32_t seed) {
  if (mode == RT_SOLID_MODE_NOISE) {
    const double f = 0.5 * (1.0 + rt_solid_noise(px, py, pz, seed));
    return f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
  }
  const double T = rt_solid_turbulence(px, py, pz, octaves, seed);
  if (mode == RT_SOLID_MODE_TURBULENCE) return T < 1.0 ? T : 1.0;
  {
    const double x = RT_SOLID_INV_2PI * (pz + 10.0 * T);
    if (!(__builtin_fabs(x) < __builtin_inf())) return 0.0; /* (NaN included) */
    const double s = x - __builtin_floor(x);
    const double m = 1.0 - __builtin_fabs(2.0 * s - 1.0);
    return m * m * (3.0 - 2.0 * m);
  }
}

#endif
