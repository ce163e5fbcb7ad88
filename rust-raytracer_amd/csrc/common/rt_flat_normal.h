// rt_flat_normal.h — shading normals of a triangle, compiled by the host (scene.cpp, the tests), the device (rt_core.h,
// rt_flat_build.hip) and the CPU tests (tests/smoothsim/).  Its bits are the contract; tests/smooth_mini.py restates it in plain Python floats.
// Every operation below is ONE IEEE f64 operation in the order written, no contraction; dot and cross are rt_quad.h's.
//
// Once per entry (rt_flat_normal_prepare).  The caller gives three vectors n0, n1, n2: the normals at Q, Q + u and Q + v.
//     all nine components +0.0 or -0.0: "no normals", the entry shades flat; its record is nine +0.0
//     otherwise every component must be finite and every dot(n_i, n_i) finite, normal and non-zero, else the entry is refused
//     the record: n_i / sqrt(dot(n_i, n_i)) per component, three divisions per vector — 9 f64 = 72 B per entry, indexed by entry k
// Per accepted hit of entry k (rt_flat_normal_shade), at shading only: the hit test, t, ids and ties are rt_quad.h's and do not change.
// P = o + d t as the test formed it, N the stored geometric normal of the entry's RtQuadRec:
//     p = P - Q    alpha = dot(w, cross(p, v))    beta = dot(w, cross(u, p))    gamma = (1 - alpha) - beta
//     m_c = (n0_c gamma + n1_c alpha) + n2_c beta                          per component c
//     mm = dot(m, m)    s = m / sqrt(mm) per component
//     (1) !(mm > 1e-24)       : s = N                (nearly opposite vertex normals; a NaN fails the test and falls back too)
//     (2) !(dot(s, N) > 0)    : s = N                (the interpolated normal points through the face)
//     front_face = dot(d, N) < 0                      (the geometric rule of rt_quad.h: inside and outside of a mesh stay what they are)
//     normal = front_face ? s : -s
//     (3) !(dot(d, normal) < 0): normal = front_face ? N : -N    (grazing: every scatter sees a normal that faces the incoming ray)
// in this order.  A scattered ray may start below the geometric face: the known price of shading normals, not corrected.
#pragma once
#include "rt_quad.h"

enum { RT_FLAT_NORMAL_FLAT = 0, RT_FLAT_NORMAL_SMOOTH = 1, RT_FLAT_NORMAL_BAD = 2 };            // rt_flat_normal_prepare
enum { RT_SHADE_FELL_MM = 1, RT_SHADE_FELL_SIDE = 2, RT_SHADE_FELL_GRAZING = 4, RT_SHADE_NO_NORMALS = 8 };  // rt_flat_normal_shade, or-ed

RT_QUAD_FN int rt_flat_normal_prepare(const double in[9], double out[9]) {
  bool zero = true;
  for (int k = 0; k < 9; ++k) zero = zero && in[k] == 0.0;
  if (zero) {
    for (int k = 0; k < 9; ++k) out[k] = 0.0;
    return RT_FLAT_NORMAL_FLAT;
  }
  for (int i = 0; i < 3; ++i) {
    const double* n = in + 3 * i;
    if (!rt_quad_finite(n[0]) || !rt_quad_finite(n[1]) || !rt_quad_finite(n[2])) return RT_FLAT_NORMAL_BAD;
    const double nn = rt_quad_dot(n, n);
    if (!(nn >= 2.2250738585072014e-308 && rt_quad_finite(nn))) return RT_FLAT_NORMAL_BAD;
    const double len = sqrt(nn);
    for (int c = 0; c < 3; ++c) out[3 * i + c] = n[c] / len;
  }
  return RT_FLAT_NORMAL_SMOOTH;
}

// a record that has normals: its first vector is a unit vector, never all zero
RT_QUAD_FN bool rt_flat_normal_present(const double rec[9]) { return !(rec[0] == 0.0 && rec[1] == 0.0 && rec[2] == 0.0); }

// alpha and beta of p = P - Q in the entry's frame: the first steps above, shared with rt_flat_image.h so the two cannot drift
RT_QUAD_FN void rt_flat_barycentric(const double u[3], const double v[3], const double w[3], const double p[3], double* alpha, double* beta) {
  double c[3];
  rt_quad_cross(p, v, c);
  *alpha = rt_quad_dot(w, c);
  rt_quad_cross(u, p, c);
  *beta = rt_quad_dot(w, c);
}

// The hit normal of a segment of direction d that hit entry r at P; rec: the entry's 72-byte record.  Returns which fallbacks were taken.
RT_QUAD_FN int rt_flat_normal_shade(const RtQuadRec& r, const double rec[9], const double d[3], const double P[3], double normal[3]) {
  const double N[3] = {r.n[0], r.n[1], r.n[2]};
  const bool front = rt_quad_dot(d, N) < 0.0;
  if (!rt_flat_normal_present(rec)) {
    for (int k = 0; k < 3; ++k) normal[k] = front ? N[k] : -N[k];
    return RT_SHADE_NO_NORMALS;
  }
  double p[3], m[3], s[3], alpha, beta;
  for (int k = 0; k < 3; ++k) p[k] = P[k] - r.q[k];
  rt_flat_barycentric(r.u, r.v, r.w, p, &alpha, &beta);
  const double gamma = (1.0 - alpha) - beta;
  for (int k = 0; k < 3; ++k) m[k] = (rec[k] * gamma + rec[3 + k] * alpha) + rec[6 + k] * beta;
  const double mm = rt_quad_dot(m, m);
  const double len = sqrt(mm);
  for (int k = 0; k < 3; ++k) s[k] = m[k] / len;
  int fell = 0;
  if (!(mm > 1e-24)) fell |= RT_SHADE_FELL_MM;
  else if (!(rt_quad_dot(s, N) > 0.0)) fell |= RT_SHADE_FELL_SIDE;
  if (fell)
    for (int k = 0; k < 3; ++k) s[k] = N[k];
  for (int k = 0; k < 3; ++k) normal[k] = front ? s[k] : -s[k];
  if (!(rt_quad_dot(d, normal) < 0.0)) {
    fell |= RT_SHADE_FELL_GRAZING;
    for (int k = 0; k < 3; ++k) normal[k] = front ? N[k] : -N[k];
  }
  return fell;
}
