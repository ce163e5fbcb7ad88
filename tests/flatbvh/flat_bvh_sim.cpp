// flat_bvh_sim.cpp — TEST TOOL, not part of the product.  The structure over the flat primitives built for the host: the
// builder and its checks (rt_tables.h), the traversal beside the scan (rt_core.h quads_hit, with the walk's counters compiled in), the
// order-free acceptance rule (rt_quad.h rt_flat_hit_tie), and the lane code of tests/lanesim/ with the structure bound.
// tests/flat_bvh_sim.py builds and binds it.
#define RT_FLAT_BVH_COUNT 1
#include <cstdint>
#include <cstring>
#include <string>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"
// The kernels' QUADS arms call flats_hit(sc, ...), which takes the structure where the scene holds one.  tests/lanesim/lane_sim.h — not to be
// edited — restates that arm with the call the kernels made before, quads_hit(o, d, ds.quads, ds.n_quads, ds.n_spheres, closest, best).  In
// THIS build that call goes through a wrapper that CHECKS it is the whole list of the scene `ds` (anything else aborts: a sub-range or
// another scene must not be tested as if it were) and then makes the kernels' call.  rt_core.h is included above: quads_hit's own
// definition is not touched.
#include <cstdlib>
namespace rtc {
inline HitCB quads_hit_of_scene(const DevScene& ds, V3 o, V3 d, QuadView view, uint32_t n, uint32_t base, double closest, int best) {
  if (view.rec != ds.quads.rec || view.lim != ds.quads.lim || n != ds.n_quads || base != ds.n_spheres) std::abort();
  return flats_hit(ds, o, d, closest, best);
}
}  // namespace rtc
#define quads_hit(o, d, view, n, base, closest, best) quads_hit_of_scene(ds, o, d, view, n, base, closest, best)
#include "../lanesim/lane_sim.h"
#undef quads_hit

using namespace lanesim;

namespace {
uint64_t (*const RENDER[16])(const RtScene&, const DevScene&, uint8_t*, float*) = {
#define FB_RENDER(k) sim_render<((k) & 8) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, ((k) & F_QUADS) != 0>
    FB_RENDER(0), FB_RENDER(1), FB_RENDER(2),  FB_RENDER(3),  FB_RENDER(4),  FB_RENDER(5),  FB_RENDER(6),  FB_RENDER(7),
    FB_RENDER(8), FB_RENDER(9), FB_RENDER(10), FB_RENDER(11), FB_RENDER(12), FB_RENDER(13), FB_RENDER(14), FB_RENDER(15)};

void put_msg(const std::string& why, char* msg, uint64_t cap) {
  if (!msg || !cap) return;
  std::strncpy(msg, why.c_str(), cap - 1);
  msg[cap - 1] = 0;
}
// the tables of a list of flat primitives alone (no scene: build_quads), with the structure when `bvh`
int flat_tables(const RtQuad* quads, uint32_t n, bool bvh, HostTables& t, char* msg, uint64_t cap) {
  std::string why = build_quads(quads, n, t);
  if (why.empty() && bvh) why = build_flat_bvh(t);
  put_msg(why, msg, cap);
  return why.empty() ? 0 : 1;
}
QuadView view_of(const HostTables& t) { return QuadView{t.quads.data(), t.quad_lim.empty() ? nullptr : t.quad_lim.data()}; }
}  // namespace

// The structure of n entries: info = {n_nodes, always-visited entries, n_tris}; nodes (cap_nodes x 64 B) and order (n x u32) when given.
// Returns 0, or 1 with the message of build_quads / build_flat_bvh.
extern "C" int fb_build(const RtQuad* quads, uint32_t n, void* nodes, uint64_t cap_nodes, uint32_t* order, uint32_t* info, char* msg, uint64_t cap_msg) {
  HostTables t;
  if (flat_tables(quads, n, true, t, msg, cap_msg)) return 1;
  info[0] = (uint32_t)t.flat_nodes.size(); info[1] = t.flat_always; info[2] = t.n_tris;
  if (nodes && cap_nodes >= t.flat_nodes.size()) std::memcpy(nodes, t.flat_nodes.data(), t.flat_nodes.size() * sizeof(FlatNode));
  if (order) std::memcpy(order, t.flat_order.data(), t.flat_order.size() * sizeof(uint32_t));
  return 0;
}

// flat_entry_box of every entry: ok[n], lo / hi [n x 3] (untouched rows where the entry is outside the preconditions)
extern "C" int fb_entry_boxes(const RtQuad* quads, uint32_t n, int32_t* ok, double* lo, double* hi) {
  HostTables t;
  if (flat_tables(quads, n, false, t, nullptr, 0)) return 1;
  for (uint32_t k = 0; k < n; ++k) ok[k] = flat_entry_box(t.quads[k], t.quad_lim.empty() ? 2.0 : t.quad_lim[k], lo + 3 * k, hi + 3 * k);
  return 0;
}

// check_flat_bvh of the caller's tables: 0 accepted, 1 refused (the message in msg)
extern "C" int fb_check(const void* nodes, uint64_t n_nodes, const uint32_t* order, uint64_t n_order, uint32_t n, char* msg, uint64_t cap_msg) {
  const FlatNode* p = static_cast<const FlatNode*>(nodes);
  const std::string why = check_flat_bvh(std::vector<FlatNode>(p, p + n_nodes), std::vector<uint32_t>(order, order + n_order), n);
  put_msg(why, msg, cap_msg);
  return why.empty() ? 0 : 1;
}

// quads_hit of n_rays rays (n x 6: o, d) with each ray's (closest_in, best_in) against the list, entry k = object id_base + k: through the
// structure (bvh != 0) or the scan.  out_best / out_t = what quads_hit returns; count[5] = {rays through the structure, rays through the
// scan inside flats_hit_bvh, box tests, entry tests, slab axes that met a NaN} of this call.
extern "C" int fb_hit_v(const RtQuad* quads, uint32_t n, uint32_t id_base, int bvh, const double* rays, const double* closest_in, const int32_t* best_in,
                        uint64_t n_rays, int32_t* out_best, double* out_t, uint64_t* count) {
  HostTables t;
  if (flat_tables(quads, n, bvh != 0, t, nullptr, 0)) return 1;
  const QuadView v = view_of(t);
  FlatBvhHeader h;   // (a list without a scene: the header as bind_host_tables writes it, in front of the builder's copy of the records)
  std::memset(&h, 0, sizeof h);
  if (bvh) {
    h.nodes = t.flat_nodes.data(); h.order = t.flat_order.data(); h.rec = t.flat_blob.data() + 1; h.lim = v.lim;
    h.n_nodes = (uint32_t)t.flat_nodes.size(); h.n_quads = n; h.id_base = id_base;
    std::memcpy(t.flat_blob.data(), &h, sizeof h);
  }
  const FlatBvhHeader* hp = bvh ? reinterpret_cast<const FlatBvhHeader*>(t.flat_blob.data()) : nullptr;
  g_flat_bvh_count = FlatBvhCount{0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n_rays; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const int b_in = best_in ? best_in[i] : -1;
    const HitCB r = bvh ? flats_hit_bvh(o, d, hp, closest_in[i], b_in) : quads_hit(o, d, v, n, id_base, closest_in[i], b_in);
    out_best[i] = r.best; out_t[i] = r.closest;
  }
  if (count) { count[0] = g_flat_bvh_count.rays_bvh; count[1] = g_flat_bvh_count.rays_scan; count[2] = g_flat_bvh_count.box_tests; count[3] = g_flat_bvh_count.entry_tests; count[4] = g_flat_bvh_count.nan_axes; }
  return 0;
}

// The surface record of accepted hits (object_surface<true>): point, normal, front for rays whose best is entry best[i] - id_base at t[i]
extern "C" int fb_surface_v(const RtQuad* quads, uint32_t n, uint32_t id_base, const double* rays, const int32_t* best, const double* t, uint64_t n_rays,
                            double* point, double* normal, int32_t* front) {
  HostTables ht;
  if (flat_tables(quads, n, false, ht, nullptr, 0)) return 1;
  for (uint64_t i = 0; i < n_rays; ++i) {
    if (best[i] < (int32_t)id_base) continue;
    const RtQuadRec& q = ht.quads[(uint32_t)best[i] - id_base];
    const double* o = rays + 6 * i; const double* d = rays + 6 * i + 3;
    double nn[3];
    front[i] = rt_quad_normal(q, d, nn);
    for (int k = 0; k < 3; ++k) { point[3 * i + k] = o[k] + d[k] * t[i]; normal[3 * i + k] = nn[k]; }
  }
  return 0;
}

// rt_flat_hit_tie beside rt_flat_hit of n rays against ONE entry (quv, lim): hit / t / P of both (zero where not accepted)
extern "C" int fb_tie_v(const double* quv, double lim, const double* rays, const double* closest, const int32_t* tie_ok, uint64_t n, int32_t* hit_a,
                        double* t_a, double* P_a, int32_t* hit_b, double* t_b, double* P_b) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  for (uint64_t i = 0; i < n; ++i) {
    double ta = 0.0, pa[3] = {0.0, 0.0, 0.0}, tb = 0.0, pb[3] = {0.0, 0.0, 0.0};
    const bool a = rt_flat_hit(r, lim, rays + 6 * i, rays + 6 * i + 3, closest[i], &ta, pa);
    const bool b = rt_flat_hit_tie(r, lim, rays + 6 * i, rays + 6 * i + 3, closest[i], tie_ok[i] != 0, &tb, pb);
    hit_a[i] = a; hit_b[i] = b; t_a[i] = a ? ta : 0.0; t_b[i] = b ? tb : 0.0;
    for (int k = 0; k < 3; ++k) { P_a[3 * i + k] = a ? pa[k] : 0.0; P_b[3 * i + k] = b ? pb[k] : 0.0; }
  }
  return 0;
}

// The frame of tests/lanesim's lane code (lane_sim_render) with the structure bound to DevScene::quads (bvh != 0) or not: rgb8 / linear
// (height x width x 3), segments.  Returns 1 when the tables were refused.
extern "C" int fb_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, int bvh, uint8_t* rgb8, float* linear,
                         uint64_t* segments, uint64_t* count) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return 1;
  if (bvh) {
    if (!build_flat_bvh(w.t).empty()) return 1;
    bind_host_tables(w.t, w.ds);
  }
  g_flat_bvh_count = FlatBvhCount{0, 0, 0, 0, 0};
  *segments = RENDER[(w.t.lights.empty() ? 0u : 8u) | (features(w) & 7u)](*sc, w.ds, rgb8, linear);
  if (count) { count[0] = g_flat_bvh_count.rays_bvh; count[1] = g_flat_bvh_count.rays_scan; count[2] = g_flat_bvh_count.box_tests; count[3] = g_flat_bvh_count.entry_tests; count[4] = g_flat_bvh_count.nan_axes; }
  return 0;
}

// the tables a device scene must hold: build_tables + build_flat_bvh of the world, nodes and order as above
extern "C" int fb_scene_tables(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, void* nodes, uint64_t cap_nodes, uint32_t* order,
                               uint32_t* info) {
  World w;
  if (build(sc, center1, quads, n_quads, w) || !build_flat_bvh(w.t).empty()) return 1;
  info[0] = (uint32_t)w.t.flat_nodes.size(); info[1] = w.t.flat_always; info[2] = w.t.n_tris;
  if (nodes && cap_nodes >= w.t.flat_nodes.size()) std::memcpy(nodes, w.t.flat_nodes.data(), w.t.flat_nodes.size() * sizeof(FlatNode));
  if (order) std::memcpy(order, w.t.flat_order.data(), w.t.flat_order.size() * sizeof(uint32_t));
  return 0;
}
