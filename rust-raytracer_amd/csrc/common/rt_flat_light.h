// rt_flat_light.h — flat primitives that emit and are sampled, compiled by the host (rt_hip_api.hip, scene.cpp, the tests),
// the device (rt_core.h) and the CPU tests (tests/flatlight/).  Its bits are the contract; tests/flat_light_mini.py restates it in plain
// Python floats.  Every operation below is ONE IEEE f64 operation in the order written, no contraction.
//
// Emitting entries.  `emit` is [n_quads][3] f32 in entry order.  An entry whose three components are all zero does not emit; any other
// entry is an EMITTER: it scatters as the reference's Light does (materials.rs:65-69: no scattered ray), its colour is `emit` instead of
// (1, 1, 1), from both faces; its own material is ignored while it emits.  Every component is finite and in [0, 1]
// (rt_flat_light_emit_check).  At most RT_MAX_FLAT_LIGHTS emitters: every sampling hit shoots one ray per light.
// The light list is the Light spheres in object order, then the emitters in entry order; n_lights is the total, in the trigger thresholds
// 1 - n_lights 0.1 / 0.05 and in the division by n_lights (raytracer.rs:100, 111-113).
//
// The aim.  Light j that is emitter entry k with resident record {Q, u, v}, shot from a hit at P whose activation has RNG node `node`:
//     c = child_node(node, j)                      (the light ray's node, as for a Light sphere)
//     w = rng(pixel, sample, c, RT_FLAT_LIGHT_SLOT)
//     a = u01_53(w.x, w.y)     b = u01_53(w.z, w.w)                  ((u64 >> 11) 2^-53 of the words (lo, hi): exact)
//     triangle only:  if (a + b > 1.0) { a = 1.0 - a;  b = 1.0 - b; }   (the sum ONE rounded addition; each difference exact or rounded once)
//     T_k = (Q_k + u_k a) + v_k b    per component k = 0, 1, 2        (two products, two additions)
//     d   = T - P                                                     (the caller's, as for a Light sphere's centre)
// Slot 0xFFFFFFFF of a node is otherwise reached only by the 2^32-th rejection of random_in_unit_sphere.  A Light sphere is aimed at as
// before: no draw.  The light ray is then an ordinary segment: its hit on the emitter, normally at t ~ 1, returns `emit`; an occluder in
// front returns what it returns.  Q, u, v are read from the entry's resident record when aiming: a lamp that rt_hip_scene_update_flats
// moved is aimed at where it now is.
#pragma once
#include "rt_quad.h"

#define RT_FLAT_LIGHT_SLOT 0xFFFFFFFFu

// (u64 >> 11) * 2^-53 of the 64-bit word hi << 32 | lo: h 2^-21 + l 2^-53 with h the top 21 bits and l the 32 below is a 53-bit number,
// both products and their sum exact (rt_core.h u01_53's form)
RT_QUAD_FN double rt_flat_light_u01(uint32_t lo, uint32_t hi) {
  const uint32_t h = hi >> 11, l = (hi << 21) | (lo >> 11);
  return (double)h * (1.0 / 2097152.0) + (double)l * (1.0 / 9007199254740992.0);
}

// the point of the entry {Q, u, v} that the four words aim at; triangle: the fold of the unit square onto a + b <= 1
RT_QUAD_FN void rt_flat_light_aim(const double Q[3], const double u[3], const double v[3], bool triangle, const uint32_t w[4], double T[3]) {
  double a = rt_flat_light_u01(w[0], w[1]), b = rt_flat_light_u01(w[2], w[3]);
  if (triangle && a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
  for (int k = 0; k < 3; ++k) T[k] = (Q[k] + u[k] * a) + v[k] * b;
}

// a component of `emit` the contract takes: finite and in [0, 1] (a NaN fails both comparisons)
RT_QUAD_FN bool rt_flat_light_component_ok(float c) { return c >= 0.0f && c <= 1.0f; }
RT_QUAD_FN bool rt_flat_light_emits(const float e[3]) { return !(e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f); }

// The table [n][3]: the lowest entry with a bad component, or n when every entry is fine; *n_emitters: the emitters among them.
RT_QUAD_FN uint32_t rt_flat_light_emit_check(const float* emit, uint32_t n, uint32_t* n_emitters) {
  uint32_t count = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const float* e = emit + 3u * (size_t)k;
    if (!rt_flat_light_component_ok(e[0]) || !rt_flat_light_component_ok(e[1]) || !rt_flat_light_component_ok(e[2])) return k;
    if (rt_flat_light_emits(e)) count++;
  }
  if (n_emitters) *n_emitters = count;
  return n;
}
