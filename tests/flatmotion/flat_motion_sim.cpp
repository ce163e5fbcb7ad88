// flat_motion_sim.cpp — TEST TOOL, not part of the product.  Flat primitives that move within the frame built for the host:
// the header (csrc/common/rt_flat_motion.h), the swept boxes and the builder (rt_flat_build.h, rt_tables.h), the traversal beside the scan
// (rt_core.h flats_walk<true>, with the walk's counters compiled in) and the QUADS ∧ MOTION lane code of tests/lanesim/lane_sim.h with the
// motion table bound as rt_hip_scene_set_flat_motion leaves it on the device.  tests/flat_motion_sim.py builds and binds it.
#define RT_FLAT_BVH_COUNT 1
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"
// tests/lanesim/lane_sim.h — not to be edited — restates the kernels' QUADS arm with the call they made before the structure,
// quads_hit(o, d, ds.quads, ...).  In THIS build that call is the kernels' own: flats_hit(ds, tb, ...), which takes the tables' shutter time.
#define quads_hit(o, d, view, n, base, closest, best) flats_hit(ds, tb, o, d, closest, best)
#include "../lanesim/lane_sim.h"
#undef quads_hit

using namespace lanesim;

namespace {
// the motion table of a list: 0, or 2 with *bad_k = the lowest refused entry; *count = the entries that move
int motion_table(const std::vector<RtQuadRec>& rec, const double* move, std::vector<double>& out, uint32_t* count, uint32_t* bad_k) {
  out.assign(4 * rec.size(), -0.0);
  *count = 0;
  for (size_t k = 0; k < rec.size(); ++k) {
    const int kind = rt_flat_motion_prepare(rec[k], move + 3 * k, &out[4 * k]);
    if (kind == RT_FLAT_MOTION_BAD) { *bad_k = (uint32_t)k; return 2; }
    *count += kind == RT_FLAT_MOTION_MOVING;
  }
  return 0;
}
// A world as the device holds it after rt_hip_scene_set_flat_motion: the records behind a header that names the motion table (the
// structure's own header, or one of its own for a scan), FLAT_MOTION_BIT, and a dv table for the spheres — all -0.0 when none moves.
struct MovingWorld {
  World w;
  std::vector<double> normals, still;
  std::vector<RtQuadRec> blob;
};
int build_moving(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const double* move, int flat_bvh,
                 MovingWorld& s, uint32_t* info) {
  World& w = s.w;
  info[0] = info[1] = 0; info[2] = 0xFFFFFFFFu;
  if (!sc || !n_quads || !build_tables(*sc, w.t, false, center1, quads, n_quads).empty()) return 1;
  uint32_t moving = 0;
  if (move) {
    if (const int rc = motion_table(w.t.quads, move, w.t.flat_motion, &moving, info + 2)) return rc;
    if (!moving) w.t.flat_motion.clear();   // all zeros: the scene is one that never had any
  }
  if (flat_bvh && !build_flat_bvh(w.t).empty()) return 1;
  fill_dev_scene(*sc, w.t, w.ds);
  bind_host_tables(w.t, w.ds);
  uint32_t smooth = 0;
  if (normals) {
    s.normals.assign(9 * (size_t)n_quads, 0.0);
    for (uint32_t k = 0; k < n_quads; ++k) {
      const int kind = rt_flat_normal_prepare(normals + 9 * (size_t)k, &s.normals[9 * (size_t)k]);
      if (kind == RT_FLAT_NORMAL_BAD) return 3;
      smooth += kind == RT_FLAT_NORMAL_SMOOTH;
    }
  }
  if (moving || smooth) {
    FlatBvhHeader* h;
    if (w.ds.n_tris & FLAT_BVH_BIT) h = const_cast<FlatBvhHeader*>(reinterpret_cast<const FlatBvhHeader*>(w.ds.quads.rec) - 1);
    else {
      s.blob.resize((size_t)n_quads + 1);
      std::memcpy(s.blob.data() + 1, w.t.quads.data(), (size_t)n_quads * sizeof(RtQuadRec));
      h = reinterpret_cast<FlatBvhHeader*>(s.blob.data());
      std::memset(h, 0, sizeof *h);
      h->rec = s.blob.data() + 1; h->lim = w.ds.quads.lim; h->n_quads = n_quads; h->id_base = w.ds.n_spheres;
      w.ds.quads.rec = s.blob.data() + 1;
    }
    if (smooth) { h->normals = s.normals.data(); w.ds.n_tris |= FLAT_NORMALS_BIT; }
    if (moving) { h->motion = w.t.flat_motion.data(); w.ds.n_tris |= FLAT_MOTION_BIT; }
  }
  if (moving && !w.ds.motion) {
    s.still.assign(4 * (size_t)(sc->n_spheres ? sc->n_spheres : 1u), -0.0);
    w.ds.motion = s.still.data();
  }
  info[0] = w.ds.n_tris; info[1] = moving;
  return 0;
}
#define FM_X8(F) {F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7)}
#define FM_RENDER(k) sim_render<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
#define FM_AOVS(k) sim_aovs<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
uint64_t (*const RENDER[8])(const RtScene&, const DevScene&, uint8_t*, float*) = FM_X8(FM_RENDER);   // bit 2: HL
void (*const AOVS[8])(const RtScene&, const DevScene&, uint32_t, float*) = FM_X8(FM_AOVS);          // bit 2: MOTION
void put_count(uint64_t* count) {
  if (!count) return;
  count[0] = g_flat_bvh_count.rays_bvh; count[1] = g_flat_bvh_count.rays_scan; count[2] = g_flat_bvh_count.box_tests;
  count[3] = g_flat_bvh_count.entry_tests; count[4] = g_flat_bvh_count.nan_axes;
}
}  // namespace

// rt_quad_prepare and rt_flat_motion_prepare of n entries: kind[n] (RT_FLAT_MOTION_*; -1: the entry itself was refused), rec[n][4]
extern "C" void fm_prepare(const double* quv, const double* move, uint32_t n, int32_t* kind, double* rec) {
  for (uint32_t k = 0; k < n; ++k) {
    RtQuadRec r;
    if (rt_quad_prepare(quv + 9 * (size_t)k, quv + 9 * (size_t)k + 3, quv + 9 * (size_t)k + 6, &r)) { kind[k] = -1; continue; }
    kind[k] = rt_flat_motion_prepare(r, move + 3 * (size_t)k, rec + 4 * (size_t)k);
  }
}

// n rays (n x 6), each with its own tau and closest-so-far, against ONE entry (quv, lim) with displacement m: the accept decision, t, P,
// the hit normal and front_face of the header (zero where not accepted).  with_table 0: the table-free test of rt_quad.h (m is ignored).
extern "C" int fm_hit_v(const double* quv, double lim, const double* m, int with_table, const double* rays, const double* tau, const double* closest,
                        uint64_t n, int32_t* hit, double* t, double* P, double* normal, int32_t* front) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  double rec[4];
  if (with_table && rt_flat_motion_prepare(r, m, rec) == RT_FLAT_MOTION_BAD) return 3;
  for (uint64_t i = 0; i < n; ++i) {
    double tt = 0.0, pp[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
    RtQuadRec at = r;
    if (with_table) rt_flat_motion_at(r, rec, tau[i], &at);
    const bool ok = with_table ? rt_flat_motion_hit_tie(r, lim, rec, tau[i], rays + 6 * i, rays + 6 * i + 3, closest[i], false, &tt, pp)
                               : rt_flat_hit(r, lim, rays + 6 * i, rays + 6 * i + 3, closest[i], &tt, pp);
    hit[i] = ok; front[i] = 0;
    if (ok) front[i] = rt_quad_normal(at, rays + 6 * i + 3, nn);
    t[i] = ok ? tt : 0.0;
    for (int k = 0; k < 3; ++k) { P[3 * i + k] = ok ? pp[k] : 0.0; normal[3 * i + k] = ok ? nn[k] : 0.0; }
  }
  return 0;
}

// flat_entry_box_swept of every entry of a list: ok[n], lo / hi [n x 3]
extern "C" int fm_boxes(const RtQuad* quads, uint32_t n, const double* move, int32_t* ok, double* lo, double* hi) {
  HostTables t;
  uint32_t moving = 0, bad = 0;
  if (!build_quads(quads, n, t).empty() || motion_table(t.quads, move, t.flat_motion, &moving, &bad)) return 1;
  for (uint32_t k = 0; k < n; ++k)
    ok[k] = flat_entry_box_swept(t.quads[k], t.quad_lim.empty() ? 2.0 : t.quad_lim[k], &t.flat_motion[4 * (size_t)k], lo + 3 * k, hi + 3 * k);
  return 0;
}

// The structure of a moving list as the host builds it: info = {n_nodes, always-visited entries, entries that move}; nodes / order /
// motion (n x 4) when given.
extern "C" int fm_build(const RtQuad* quads, uint32_t n, const double* move, void* nodes, uint64_t cap_nodes, uint32_t* order, double* motion, uint32_t* info) {
  HostTables t;
  uint32_t moving = 0, bad = 0;
  if (!build_quads(quads, n, t).empty() || motion_table(t.quads, move, t.flat_motion, &moving, &bad)) return 1;
  if (!moving) t.flat_motion.clear();
  if (!build_flat_bvh(t).empty()) return 1;
  info[0] = (uint32_t)t.flat_nodes.size(); info[1] = t.flat_always; info[2] = moving;
  if (nodes && cap_nodes >= t.flat_nodes.size()) std::memcpy(nodes, t.flat_nodes.data(), t.flat_nodes.size() * sizeof(FlatNode));
  if (order) std::memcpy(order, t.flat_order.data(), t.flat_order.size() * sizeof(uint32_t));
  if (motion && moving) std::memcpy(motion, t.flat_motion.data(), t.flat_motion.size() * sizeof(double));
  return 0;
}

// flats_walk<true> of n_rays rays, each with its tau, closest_in and best_in, against a moving list (entry k = object id_base + k):
// through the structure (bvh != 0) or the scan.  count[5] as tests/flatbvh's.
extern "C" int fm_list_hit(const RtQuad* quads, uint32_t n, const double* move, uint32_t id_base, int bvh, const double* rays, const float* tau,
                           const double* closest_in, const int32_t* best_in, uint64_t n_rays, int32_t* out_best, double* out_t, uint64_t* count) {
  HostTables t;
  uint32_t moving = 0, bad = 0;
  if (!build_quads(quads, n, t).empty() || motion_table(t.quads, move, t.flat_motion, &moving, &bad)) return 1;
  if (bvh && !build_flat_bvh(t).empty()) return 1;
  std::vector<RtQuadRec> blob((size_t)n + 1);
  std::memcpy(blob.data() + 1, t.quads.data(), (size_t)n * sizeof(RtQuadRec));
  FlatBvhHeader h;
  std::memset(&h, 0, sizeof h);
  h.nodes = t.flat_nodes.data(); h.order = t.flat_order.data(); h.rec = blob.data() + 1; h.lim = t.quad_lim.empty() ? nullptr : t.quad_lim.data();
  h.n_nodes = (uint32_t)t.flat_nodes.size(); h.n_quads = n; h.id_base = id_base; h.motion = t.flat_motion.data();
  std::memcpy(blob.data(), &h, sizeof h);
  g_flat_bvh_count = FlatBvhCount{0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n_rays; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const HitCB r = flats_walk<true>(o, d, reinterpret_cast<const FlatBvhHeader*>(blob.data()), bvh ? 1u : 0u, (double)tau[i], closest_in[i], best_in ? best_in[i] : -1);
    out_best[i] = r.best; out_t[i] = r.closest;
  }
  put_count(count);
  return 0;
}

// What rt_hip_flat_shutter_probe runs on the device (include/rt_abi_test_flat_motion.h), the same two calls in this build: the arguments of
// fm_list_hit plus normals (null or n x 9; move may be null too) -> flats_hit through motion_tables at the ray's tau — an f32, widened where
// the kernels widen it — and, for a newly accepted flat entry, object_surface<true>: t, P, the normal, front_face and the origin left in
// g.cx, g.cy, g.cz.  out_best is always written, the rest only on such a hit.  The scene is the one rt_hip_scene_set_flat_normals /
// _set_flat_motion leave: the bits of n_tris behind which the kernels choose, the header in front of the records, a sphere table in which
// nothing moves.  1: the list was refused; 3: a normal was.
extern "C" int fm_list_surface(const RtQuad* quads, uint32_t n, const double* move, const double* normals, uint32_t id_base, int bvh, const double* rays,
                               const float* tau, const double* closest_in, const int32_t* best_in, uint64_t n_rays, int32_t* out_best, double* out_t,
                               double* out_P, double* out_normal, int32_t* out_front, double* out_origin, uint64_t* count) {
  HostTables t;
  uint32_t moving = 0, bad = 0, smooth = 0;
  if (!n || !build_quads(quads, n, t).empty()) return 1;
  if (move && motion_table(t.quads, move, t.flat_motion, &moving, &bad)) return 1;
  if (!moving) t.flat_motion.clear();
  if (bvh && !build_flat_bvh(t).empty()) return 1;
  std::vector<double> nrec;
  if (normals) {
    nrec.assign(9 * (size_t)n, 0.0);
    for (uint32_t k = 0; k < n; ++k) {
      const int kind = rt_flat_normal_prepare(normals + 9 * (size_t)k, &nrec[9 * (size_t)k]);
      if (kind == RT_FLAT_NORMAL_BAD) return 3;
      smooth += kind == RT_FLAT_NORMAL_SMOOTH;
    }
  }
  std::vector<RtQuadRec> blob((size_t)n + 1);
  std::memcpy(blob.data() + 1, t.quads.data(), (size_t)n * sizeof(RtQuadRec));
  FlatBvhHeader h;
  std::memset(&h, 0, sizeof h);
  h.nodes = t.flat_nodes.data(); h.order = t.flat_order.data(); h.rec = blob.data() + 1; h.lim = t.quad_lim.empty() ? nullptr : t.quad_lim.data();
  h.n_nodes = (uint32_t)t.flat_nodes.size(); h.n_quads = n; h.id_base = id_base;
  h.normals = smooth ? nrec.data() : nullptr; h.motion = moving ? t.flat_motion.data() : nullptr;
  std::memcpy(blob.data(), &h, sizeof h);
  const std::vector<double> still(4 * (size_t)(id_base ? id_base : 1u), -0.0);
  DevScene ds;
  std::memset(&ds, 0, sizeof ds);
  ds.n_spheres = id_base; ds.quads = QuadView{blob.data() + 1, h.lim}; ds.n_quads = n; ds.motion = still.data();
  ds.n_tris = (bvh ? FLAT_BVH_BIT : 0u) | (smooth ? FLAT_NORMALS_BIT : 0u) | (moving ? FLAT_MOTION_BIT : 0u);
  const GlobalTables none{nullptr, nullptr};
  g_flat_bvh_count = FlatBvhCount{0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n_rays; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const auto tb = motion_tables(none, ds.motion, tau ? tau[i] : 0.0f);
    const int held = best_in ? best_in[i] : -1;
    const HitCB r = flats_hit(ds, tb, o, d, closest_in[i], held);
    out_best[i] = r.best;
    if (r.best == held || r.best < 0 || (uint32_t)r.best < id_base || (uint32_t)r.best - id_base >= n) continue;
    SphereGeom g;
    const Surface s = object_surface<true>(ds, tb, o, d, r.closest, (uint32_t)r.best, 0.0, g);
    out_t[i] = r.closest;
    out_P[3 * i] = s.point.x; out_P[3 * i + 1] = s.point.y; out_P[3 * i + 2] = s.point.z;
    out_normal[3 * i] = s.normal.x; out_normal[3 * i + 1] = s.normal.y; out_normal[3 * i + 2] = s.normal.z;
    out_front[i] = s.front_face ? 1 : 0;
    out_origin[3 * i] = g.cx; out_origin[3 * i + 1] = g.cy; out_origin[3 * i + 2] = g.cz;
  }
  put_count(count);
  return 0;
}

// The frame of the QUADS lane code (MOTION where something moves).  normals: null or n x 9; move: null or n x 3.  info = {DevScene::n_tris,
// entries that move, the lowest refused entry}.
extern "C" int fm_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const double* move, int flat_bvh,
                         uint8_t* rgb8, float* linear, uint64_t* segments, uint32_t* info, uint64_t* count) {
  MovingWorld s;
  if (const int rc = build_moving(sc, center1, quads, n_quads, normals, move, flat_bvh, s, info)) return rc;
  const World& w = s.w;
  g_flat_bvh_count = FlatBvhCount{0, 0, 0, 0, 0};
  *segments = RENDER[(w.t.lights.empty() ? 0u : 4u) | (features(w) & 3u)](*sc, w.ds, rgb8, linear);
  put_count(count);
  return 0;
}
// The first-hit records of n samples per pixel (height x width x 8 f32) and the surface record of every pixel (height x width x 16 B).
extern "C" int fm_aovs(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const double* move, int flat_bvh,
                       uint32_t n, float* out, void* surface) {
  MovingWorld s;
  uint32_t info[3];
  if (const int rc = build_moving(sc, center1, quads, n_quads, normals, move, flat_bvh, s, info)) return rc;
  AOVS[(s.w.ds.motion ? 4u : 0u) | (features(s.w) & 3u)](*sc, s.w.ds, n, out);
  if (surface) {
    SurfRec* o = static_cast<SurfRec*>(surface);
    if (s.w.ds.motion) { if (s.w.ds.medium) sim_surface<true, true, true>(*sc, s.w.ds, o); else sim_surface<true, false, true>(*sc, s.w.ds, o); }
    else { if (s.w.ds.medium) sim_surface<false, true, true>(*sc, s.w.ds, o); else sim_surface<false, false, true>(*sc, s.w.ds, o); }
  }
  return 0;
}
