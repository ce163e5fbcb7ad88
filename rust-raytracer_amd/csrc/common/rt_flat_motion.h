// rt_flat_motion.h — flat primitives that move while the shutter is open, compiled by the host (rt_tables.h, the tests),
// the device (rt_core.h, rt_flat_build.hip) and the CPU tests (tests/flatmotion/).  Its bits are the contract; tests/flat_motion_mini.py
// restates it in plain Python floats.  Every operation below is ONE IEEE f64 operation in the order written, no contraction; dot is
// rt_quad.h's.
//
// An entry may carry a displacement m over the open shutter: at shutter time tau (DESIGN.md §14's tau, the sample's) it is the same
// primitive translated by m tau.  u, v and the normal do not change with tau.
// Once per entry (rt_flat_motion_prepare), where its record is made: the 32-byte record {m0, m1, m2, Dm}, Dm = dot(N, m) with the N of the
// entry's RtQuadRec.  An entry whose three components are all zero stores -0.0 in all four slots: x + (-0.0) tau gives x's own bits back
// for every tau >= 0 (+0 and -0 included), so a static entry of a moving scene is tested on exactly the bits it has in a scene without the
// table (§14's trick).  Refused: a component of m that is not finite, or a q_k + m_k that is not finite.
// Per segment (rt_flat_motion_at), the entry's record at tau:
//     Dtau = D + Dm tau        Qtau_k = q_k + m_k tau per component          u, v, N, w: the record's
// and every step of rt_quad.h's test runs on that record: den = dot(N, d), t = (Dtau - dot(N, o)) / den, the accept rules,
// P = o + d t, p = P - Qtau, alpha, beta, the limit test, front_face and the normal.  Everything that uses q as a frame uses Qtau: the
// pattern centre of a Checker or Noise entry (§16) and the barycentric weights of the shading normals (§25).
#pragma once
#include "rt_quad.h"

enum { RT_FLAT_MOTION_STILL = 0, RT_FLAT_MOTION_MOVING = 1, RT_FLAT_MOTION_BAD = 2 };  // rt_flat_motion_prepare

RT_QUAD_FN int rt_flat_motion_prepare(const RtQuadRec& r, const double m[3], double out[4]) {
  for (int k = 0; k < 3; ++k)
    if (!rt_quad_finite(m[k]) || !rt_quad_finite(r.q[k] + m[k])) return RT_FLAT_MOTION_BAD;
  if (m[0] == 0.0 && m[1] == 0.0 && m[2] == 0.0) {
    for (int k = 0; k < 4; ++k) out[k] = -0.0;
    return RT_FLAT_MOTION_STILL;
  }
  for (int k = 0; k < 3; ++k) out[k] = m[k];
  out[3] = rt_quad_dot(r.n, m);
  return RT_FLAT_MOTION_MOVING;
}

// a record of an entry that moves (a still entry's is four -0.0)
RT_QUAD_FN bool rt_flat_motion_present(const double rec[4]) { return !(rec[0] == 0.0 && rec[1] == 0.0 && rec[2] == 0.0); }

// the entry's record at shutter time tau
RT_QUAD_FN void rt_flat_motion_at(const RtQuadRec& r, const double rec[4], double tau, RtQuadRec* out) {
  for (int k = 0; k < 3; ++k) {
    out->q[k] = r.q[k] + rec[k] * tau;
    out->u[k] = r.u[k]; out->v[k] = r.v[k]; out->n[k] = r.n[k]; out->w[k] = r.w[k];
  }
  out->d = r.d + rec[3] * tau;
}

// the far end of the motion, q (+) m: one addition per component (what the swept box of rt_flat_build.h is made from)
RT_QUAD_FN void rt_flat_motion_end(const RtQuadRec& r, const double rec[4], RtQuadRec* out) {
  *out = r;
  for (int k = 0; k < 3; ++k) out->q[k] = r.q[k] + rec[k];
}

// rt_flat_hit_tie (and with tie_ok false rt_flat_hit) of the entry at shutter time tau
RT_QUAD_FN bool rt_flat_motion_hit_tie(const RtQuadRec& r, double lim, const double rec[4], double tau, const double o[3], const double d[3],
                                       double closest, bool tie_ok, double* t_out, double P[3]) {
  RtQuadRec at;
  rt_flat_motion_at(r, rec, tau, &at);
  return rt_flat_hit_tie(at, lim, o, d, closest, tie_ok, t_out, P);
}
