// rt_quad.h — the flat parallelogram of DESIGN.md §20 ("Quadrilaterals" of The Next Week) and the triangle of §21, compiled by the host
// (rt_tables.h, scene.cpp), the device (rt_core.h) and the CPU tests (tests/lanesim/, tests/trisim/).  Its bits are the contract;
// tests/quad_mini.py and tests/tri_mini.py restate it in plain Python floats.
//
// A quad is Q, u, v (f64 x 3 each): the points Q + a u + b v with 0 <= a, b <= 1, two-sided.  Every operation below is ONE IEEE f64
// operation in the order written, no contraction (every build has -ffp-contract=off):
//     dot(p, q)   = (p0 q0 + p1 q1) + p2 q2
//     cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)          (rt_abi.h, rt_hip_reproject's)
// Once per quad (rt_quad_prepare: the host at creation, the device when the flat primitives of a resident scene move):
//     n = cross(u, v)    nn = dot(n, n)    len = sqrt(nn)
//     N = n / len per component    D = dot(N, Q)    w = n / nn per component
// A quad whose q, u or v has a non-finite component, or whose nn is zero, subnormal or not finite, is refused.
// Per segment with origin o, direction d (not normalised) and the closest hit so far `closest` (rt_quad_hit):
//     den = dot(N, d)                       fabs(den) < 1e-8: no hit (a NaN den fails every later comparison: no hit either)
//     t = (D - dot(N, o)) / den             accepted only if t > 0.001 and t < closest   (strict: on a tie the earlier object stays)
//     P = o + d t per component (ray.rs:18-20)    p = P - Q
//     alpha = dot(w, cross(p, v))    beta = dot(w, cross(u, p))     accepted iff 0 <= alpha, alpha <= 1, 0 <= beta, beta <= 1
// The record of an accepted hit: point P, front_face = dot(d, N) < 0, normal = front_face ? N : -N, and t.
//
// Triangles.  A flat primitive is Q, u, v plus a SHAPE: parallelogram (the quad above) or triangle, the points
// Q + a u + b v with 0 <= a, 0 <= b, a + b <= 1, two-sided.  rt_quad_prepare, every step of the test up to and including alpha and
// beta, the record and the 128-byte RtQuadRec are the quad's.  Each primitive has a limit `lim`: 2.0 for a parallelogram, 1.0 for a
// triangle, and a hit is accepted (rt_flat_hit) iff
//     0 <= alpha, alpha <= 1, 0 <= beta, beta <= 1 and alpha + beta <= lim          (the sum: ONE IEEE f64 addition, no contraction)
// With alpha, beta in [0, 1] the rounded sum never exceeds 2, so lim = 2 accepts exactly what rt_quad_hit accepts; for a triangle
// alpha <= 1 and beta <= 1 follow from the other three comparisons: one rule serves both shapes.  A NaN fails every comparison.
// front_face comes from N = cross(u, v) / |cross(u, v)|: a closed Glass mesh needs outward (counter-clockwise) winding.  NOT
// watertight: two triangles that share an edge each round their own alpha and beta; the test IS this arithmetic.
//
// The list.  For a segment (o, d) and the (closest_in, best_in) the spheres left, let A be the entries k that
// rt_flat_hit(rec_k, lim_k, o, d, closest_in, ...) accepts (lim_k = 2.0 in a scene without a triangle).  The full scan returns the entry of
// A with the smallest (t_k, k) in lexicographic order, or its input unchanged when A is empty; t_k does not depend on `closest`, so neither
// does the result depend on the visiting order.  Any structure over the entries (rt_core.h flats_hit_bvh) returns exactly this: a sphere
// still beats a flat entry on an equal t, an earlier entry a later one, and a NaN fails every comparison (rt_flat_hit_tie below).
// PRECONDITION: best_in is what the spheres left — a sphere's id or a miss, never a flat entry's.
// (The kernels keep to it.  The moving list — rt_core.h flats_walk<true>, scan and structure alike — is probed beyond it, DESIGN.md §30: a flat
// entry held on entry takes part in the order like any other, so an entry of a SMALLER index takes an equal t from it and nothing else does.)
//
// An axis-aligned box (rt_box_quads) with corners min = (x0, y0, z0) and max = (x1, y1, z1), dx = x1 - x0, dy = y1 - y0, dz = z1 - z0
// (one subtraction each; a negation is exact; every other component is +0.0), is these six quads in this order:
//     0 front  (z = z1): Q = (x0, y0, z1)  u = ( dx, 0, 0)  v = (0, dy,   0)
//     1 right  (x = x1): Q = (x1, y0, z1)  u = (0, 0, -dz)  v = (0, dy,   0)
//     2 back   (z = z0): Q = (x1, y0, z0)  u = (-dx, 0, 0)  v = (0, dy,   0)
//     3 left   (x = x0): Q = (x0, y0, z0)  u = (0, 0,  dz)  v = (0, dy,   0)
//     4 top    (y = y1): Q = (x0, y1, z1)  u = ( dx, 0, 0)  v = (0, 0,  -dz)
//     5 bottom (y = y0): Q = (x0, y0, z0)  u = ( dx, 0, 0)  v = (0, 0,   dz)
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef RT_QUAD_FN
#if defined(__HIPCC__)
#define RT_QUAD_FN __host__ __device__ inline
#else
#define RT_QUAD_FN inline
#endif
#endif

// The resident record of one quad, 128 B, as the kernels read it (rt_hip_scene_table "quads"): the caller's three vectors and the
// host's constants.
struct RtQuadRec {
  double q[3], u[3], v[3];
  double n[3];  // N, the unit normal
  double w[3];
  double d;     // D
};

RT_QUAD_FN double rt_quad_dot(const double p[3], const double q[3]) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
RT_QUAD_FN void rt_quad_cross(const double a[3], const double b[3], double out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
}
RT_QUAD_FN bool rt_quad_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// The per-quad constants, on the host (creation) and on the device (rt_flat_build.hip: rt_hip_scene_update_flats): sqrt and /
// are correctly rounded on both, so the record's bits are the same.  0: fine; 1: a non-finite component of q, u or v; 2: degenerate (nn
// zero, subnormal or not finite).
RT_QUAD_FN int rt_quad_prepare(const double q[3], const double u[3], const double v[3], RtQuadRec* out) {
  for (int k = 0; k < 3; ++k)
    if (!rt_quad_finite(q[k]) || !rt_quad_finite(u[k]) || !rt_quad_finite(v[k])) return 1;
  double n[3];
  rt_quad_cross(u, v, n);
  const double nn = rt_quad_dot(n, n);
  if (!(nn >= 2.2250738585072014e-308 && rt_quad_finite(nn))) return 2;
  const double len = sqrt(nn);
  for (int k = 0; k < 3; ++k) { out->q[k] = q[k]; out->u[k] = u[k]; out->v[k] = v[k]; out->n[k] = n[k] / len; out->w[k] = n[k] / nn; }
  out->d = rt_quad_dot(out->n, q);
  return 0;
}

// One segment against one quad: true and (t, P) when the contract accepts the hit.
RT_QUAD_FN bool rt_quad_hit(const RtQuadRec& r, const double o[3], const double d[3], double closest, double* t_out, double P[3]) {
  const double den = rt_quad_dot(r.n, d);
  if (fabs(den) < 1e-8) return false;
  const double t = (r.d - rt_quad_dot(r.n, o)) / den;
  if (!(t > 0.001 && t < closest)) return false;
  double p[3], c[3];
  for (int k = 0; k < 3; ++k) { P[k] = o[k] + d[k] * t; p[k] = P[k] - r.q[k]; }
  rt_quad_cross(p, r.v, c);
  const double alpha = rt_quad_dot(r.w, c);
  rt_quad_cross(r.u, p, c);
  const double beta = rt_quad_dot(r.w, c);
  if (!(0.0 <= alpha && alpha <= 1.0 && 0.0 <= beta && beta <= 1.0)) return false;
  *t_out = t;
  return true;
}

// One segment against one flat primitive of limit `lim` (2.0: parallelogram, 1.0: triangle): rt_quad_hit's steps and bits, plus the
// comparison of alpha + beta with lim.
RT_QUAD_FN bool rt_flat_hit(const RtQuadRec& r, double lim, const double o[3], const double d[3], double closest, double* t_out, double P[3]) {
  const double den = rt_quad_dot(r.n, d);
  if (fabs(den) < 1e-8) return false;
  const double t = (r.d - rt_quad_dot(r.n, o)) / den;
  if (!(t > 0.001 && t < closest)) return false;
  double p[3], c[3];
  for (int k = 0; k < 3; ++k) { P[k] = o[k] + d[k] * t; p[k] = P[k] - r.q[k]; }
  rt_quad_cross(p, r.v, c);
  const double alpha = rt_quad_dot(r.w, c);
  rt_quad_cross(r.u, p, c);
  const double beta = rt_quad_dot(r.w, c);
  if (!(0.0 <= alpha && alpha <= 1.0 && 0.0 <= beta && beta <= 1.0)) return false;
  if (!(alpha + beta <= lim)) return false;
  *t_out = t;
  return true;
}

// The order-free form of rt_flat_hit: its steps and bits, repeated, with the range test
//     t > 0.001 and (t < closest or (tie_ok and t == closest)).
// A traversal that meets the entries in any order sets tie_ok when the hit it holds is a flat entry of a LARGER index than this one: the
// smaller index then takes an equal t, as it does in the scan.  With tie_ok false this is rt_flat_hit in decision and every output bit.
RT_QUAD_FN bool rt_flat_hit_tie(const RtQuadRec& r, double lim, const double o[3], const double d[3], double closest, bool tie_ok, double* t_out,
                                double P[3]) {
  const double den = rt_quad_dot(r.n, d);
  if (fabs(den) < 1e-8) return false;
  const double t = (r.d - rt_quad_dot(r.n, o)) / den;
  if (!(t > 0.001 && (t < closest || (tie_ok && t == closest)))) return false;
  double p[3], c[3];
  for (int k = 0; k < 3; ++k) { P[k] = o[k] + d[k] * t; p[k] = P[k] - r.q[k]; }
  rt_quad_cross(p, r.v, c);
  const double alpha = rt_quad_dot(r.w, c);
  rt_quad_cross(r.u, p, c);
  const double beta = rt_quad_dot(r.w, c);
  if (!(0.0 <= alpha && alpha <= 1.0 && 0.0 <= beta && beta <= 1.0)) return false;
  if (!(alpha + beta <= lim)) return false;
  *t_out = t;
  return true;
}

// front_face and the hit normal of a segment of direction d that hit the quad
RT_QUAD_FN bool rt_quad_normal(const RtQuadRec& r, const double d[3], double normal[3]) {
  const bool front = rt_quad_dot(d, r.n) < 0.0;
  for (int k = 0; k < 3; ++k) normal[k] = front ? r.n[k] : -r.n[k];
  return front;
}

// the six quads of an axis-aligned box, out[6][9] = {q, u, v} each, in the order of the header
inline void rt_box_quads(const double mn[3], const double mx[3], double out[6][9]) {
  const double dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
  const double x0 = mn[0], y0 = mn[1], z0 = mn[2], x1 = mx[0], y1 = mx[1], z1 = mx[2];
  const double t[6][9] = {{x0, y0, z1, dx, 0.0, 0.0, 0.0, dy, 0.0},  {x1, y0, z1, 0.0, 0.0, -dz, 0.0, dy, 0.0},
                          {x1, y0, z0, -dx, 0.0, 0.0, 0.0, dy, 0.0}, {x0, y0, z0, 0.0, 0.0, dz, 0.0, dy, 0.0},
                          {x0, y1, z1, dx, 0.0, 0.0, 0.0, 0.0, -dz}, {x0, y0, z0, dx, 0.0, 0.0, 0.0, 0.0, dz}};
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < 9; ++k) out[i][k] = t[i][k];
}
