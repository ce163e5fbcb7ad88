// CPU build of the quads (tests/test_quad_cpu.py; tests only): csrc/common/rt_quad.h built for the host, ray by ray, the tables rt_tables.h
// builds for a scene with quads, and the per-lane code of the QUADS kernels (rt_core.h quads_hit behind hit_world_grid, lane_shade<MEDIUM,
// SOLID, true>, the QUADS arms of aov_pixel and surface_pixel) one lane at a time — what the QUADS megakernels, rt_aov_quads and
// rt_surface_quads run, without a GPU.
#include <cstdint>
#include <cstring>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"

using namespace rtc;

namespace {
struct World {
  HostTables t;
  DevScene ds;
};
int build(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, World& w) {
  if (!build_tables(*sc, w.t, false, center1, quads, n_quads).empty()) return 1;
  fill_dev_scene(*sc, w.t, w.ds);
  w.ds.geom = w.t.geom.data();
  w.ds.matc = w.t.matc.data();
  w.ds.mat = w.t.mat.data();
  w.ds.lights = w.t.lights.data();
  w.ds.cell_word = w.t.cell_word.data();
  w.ds.cell_items = w.t.grid.wide ? reinterpret_cast<const uint16_t*>(w.t.cell_items32.data()) : w.t.cell_items.data();
  w.ds.large = w.t.large.data();
  w.ds.large_geom = w.t.large_geom.data();
  w.ds.motion = w.t.motion.empty() ? nullptr : w.t.motion.data();
  w.ds.medium = w.t.medium.empty() ? nullptr : w.t.medium.data();
  w.ds.quads = w.t.quads.empty() ? nullptr : w.t.quads.data();
  w.ds.n_quads = (uint32_t)w.t.quads.size();
  return 0;
}
template <typename V>
void put(std::vector<uint8_t>& blob, const V& v) {
  const uint64_t bytes = v.size() * sizeof(typename V::value_type);
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&bytes);
  blob.insert(blob.end(), p, p + 8);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(v.data());
  blob.insert(blob.end(), d, d + bytes);
}
}  // namespace

// rt_quad_prepare of n quads, quv = n x 9 (q, u, v): rec = n x 16 doubles (RtQuadRec), status[n] = its return value
extern "C" void quad_prepare_v(const double* quv, uint64_t n, double* rec, int32_t* status) {
  for (uint64_t i = 0; i < n; ++i) {
    RtQuadRec r;
    std::memset(&r, 0, sizeof r);
    status[i] = rt_quad_prepare(quv + 9 * i, quv + 9 * i + 3, quv + 9 * i + 6, &r);
    std::memcpy(rec + 16 * i, &r, sizeof r);
  }
}

// rt_quad_hit and rt_quad_normal of n rays (rays = n x 6: o, d) against ONE quad (quv = 9 doubles) with closest[n]:
// hit[n], t[n], P[n x 3], normal[n x 3], front[n] (zero where the ray does not hit).  Returns rt_quad_prepare's status.
extern "C" int quad_hit_v(const double* quv, const double* rays, const double* closest, uint64_t n, int32_t* hit, double* t, double* P, double* normal,
                          int32_t* front) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  for (uint64_t i = 0; i < n; ++i) {
    double tt = 0.0, pp[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
    const bool h = rt_quad_hit(r, rays + 6 * i, rays + 6 * i + 3, closest[i], &tt, pp);
    bool f = false;
    if (h) f = rt_quad_normal(r, rays + 6 * i + 3, nn);
    hit[i] = h; t[i] = h ? tt : 0.0; front[i] = f;
    for (int k = 0; k < 3; ++k) { P[3 * i + k] = h ? pp[k] : 0.0; normal[3 * i + k] = nn[k]; }
  }
  return 0;
}

// the six quads of a box, out = 6 x 9
extern "C" void quad_box(const double* mn, const double* mx, double* out) {
  double q[6][9];
  rt_box_quads(mn, mx, q);
  std::memcpy(out, q, sizeof q);
}

// Every table build_tables fills, length-prefixed and back to back (geom, mat, matc, cell_word, cell_items, cell_items32, large, large_geom,
// motion, medium, lights, quads, then the GridDesc and the counts), into out (cap bytes).  Returns the blob's size, or -1 when build_tables
// refused the world; info = {n_solids, n_media, n_moving, wide, n_quads, simple_colour}.
extern "C" int64_t quad_tables(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t* info, uint8_t* out, uint64_t cap) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return -1;
  const HostTables& t = w.t;
  info[0] = t.n_solids; info[1] = t.n_media; info[2] = t.n_moving; info[3] = t.grid.wide; info[4] = (uint32_t)t.quads.size(); info[5] = t.simple_colour;
  std::vector<uint8_t> blob;
  put(blob, t.geom); put(blob, t.mat); put(blob, t.matc); put(blob, t.cell_word); put(blob, t.cell_items); put(blob, t.cell_items32);
  put(blob, t.large); put(blob, t.large_geom); put(blob, t.motion); put(blob, t.medium); put(blob, t.lights); put(blob, t.quads);
  const uint8_t* g = reinterpret_cast<const uint8_t*>(&t.grid);
  blob.insert(blob.end(), g, g + sizeof t.grid);
  if (out && cap >= blob.size()) std::memcpy(out, blob.data(), blob.size());
  return (int64_t)blob.size();
}
// why build_tables refused the world ("" when it did not), into msg (cap bytes)
extern "C" void quad_tables_error(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, char* msg, uint64_t cap) {
  HostTables t;
  const std::string why = build_tables(*sc, t, false, center1, quads, n_quads);
  std::strncpy(msg, why.c_str(), cap - 1);
  msg[cap - 1] = 0;
}

// hit_world of the QUADS kernels for n rays (n x 6) through the scene's own tables: best[n] (object id, -1: a miss), t[n]
extern "C" int quad_sim_hits(const RtScene* sc, const RtQuad* quads, uint32_t n_quads, const double* rays, uint64_t n, int32_t* best_out, double* t_out) {
  World w;
  if (build(sc, nullptr, quads, n_quads, w)) return 1;
  const GlobalTables base{w.ds.geom, w.ds.matc};
  for (uint64_t i = 0; i < n; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    double closest = T_MAX;
    int best = -1;
    uint32_t ne = 0, ns = 0;
    hit_world_grid(w.ds, base, o, d, closest, best, ne, ns);
    const HitCB r = quads_hit(o, d, w.ds.quads, w.ds.n_quads, w.ds.n_spheres, closest, best);
    best_out[i] = r.best; t_out[i] = r.best >= 0 ? r.closest : 0.0;
  }
  return 0;
}

namespace {
template <bool HL, bool MEDIUM>
uint64_t sim_render(const RtScene& sc, const World& w, uint8_t* rgb8, float* linear) {
  const DevScene& ds = w.ds;
  const GlobalTables base{ds.geom, ds.matc};
  uint64_t segs = 0;
  for (uint32_t y = 0; y < sc.height; ++y)
    for (uint32_t x = 0; x < sc.width; ++x) {
      Lane<HL, false> L;
      std::memset(&L, 0, sizeof L);
      LightStack<HL> light_stack;
      LightParked light_parked;
      lane_attach_light_state(L, light_stack, &light_parked);
      L.ra.pixel = y * sc.width + x; L.ra.k0 = ds.seed_lo; L.ra.k1 = ds.seed_hi;
      unsigned long long facc[3] = {0ull, 0ull, 0ull};
      for (L.s = 0; L.s < sc.samples_per_pixel && sc.max_depth != 0; ++L.s) {
        lane_begin_sample(ds, L, x, y);
        const float tau = ds.motion ? sample_time(L.ra) : 0.0f;
        for (;;) {
          double closest = T_MAX;
          int best = -1;
          uint32_t ns = 0;
          L.n_segments++;
          const MediumCtx mc{ds.medium, L.ra, L.node};
          int st;
          if (ds.motion) {
            const auto tb = motion_tables(base, ds.motion, tau);
            hit_world_grid<MEDIUM>(ds, tb, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            const HitCB r = quads_hit(L.o, L.d, ds.quads, ds.n_quads, ds.n_spheres, closest, best);
            st = lane_shade<MEDIUM, true, true>(ds, tb, L, r.best, r.closest);
          } else {
            hit_world_grid<MEDIUM>(ds, base, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            const HitCB r = quads_hit(L.o, L.d, ds.quads, ds.n_quads, ds.n_spheres, closest, best);
            st = lane_shade<MEDIUM, true, true>(ds, base, L, r.best, r.closest);
          }
          if (st == LANE_FINISHED) break;
        }
        for (int k = 0; k < 3; ++k) facc[k] += sample_to_fixed(L.val[k]);
      }
      for (int k = 0; k < 3; ++k) {
        const float lin = fixed_to_mean(facc[k], sc.samples_per_pixel);
        const size_t o = ((size_t)y * sc.width + x) * 3 + k;
        linear[o] = lin;
        rgb8[o] = f32_to_u8(sqrtf(lin));
      }
      segs += L.n_segments;
    }
  return segs;
}
template <bool MOTION, bool MEDIUM>
void sim_aovs(const RtScene& sc, const World& w, uint32_t n, float* out) {
  const GlobalTables base{w.ds.geom, w.ds.matc};
  for (uint32_t y = 0; y < sc.height; ++y)
    for (uint32_t x = 0; x < sc.width; ++x) aov_pixel<false, MOTION, MEDIUM, true, true>(w.ds, base, x, y, n, out + 8 * ((size_t)y * sc.width + x));
}
template <bool MOTION, bool MEDIUM>
void sim_surface(const RtScene& sc, const World& w, uint32_t* ids, uint32_t* kinds, double* ts) {
  const GlobalTables base{w.ds.geom, w.ds.matc};
  for (uint32_t y = 0; y < sc.height; ++y)
    for (uint32_t x = 0; x < sc.width; ++x) {
      const SurfRec r = surface_pixel<MOTION, MEDIUM, true>(w.ds, base, x, y);
      const size_t p = (size_t)y * sc.width + x;
      ids[p] = r.id; kinds[p] = r.kind; ts[p] = r.t;
    }
}
}  // namespace

// The pinhole camera; static or moving spheres; with or without media and solids; lit or unlit.  -> rgb8 / linear (height x width x 3), segments.
extern "C" int quad_sim_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint8_t* rgb8, float* linear, uint64_t* segments) {
  World w;
  if (build(sc, center1, quads, n_quads, w) || !w.ds.n_quads) return 1;
  const bool hl = !w.t.lights.empty();
  if (w.ds.medium) *segments = hl ? sim_render<true, true>(*sc, w, rgb8, linear) : sim_render<false, true>(*sc, w, rgb8, linear);
  else *segments = hl ? sim_render<true, false>(*sc, w, rgb8, linear) : sim_render<false, false>(*sc, w, rgb8, linear);
  return 0;
}

// The first-hit records of n samples per pixel (height x width x 8 f32), the pinhole camera.
extern "C" int quad_sim_aovs(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t n, float* out) {
  World w;
  if (build(sc, center1, quads, n_quads, w) || !w.ds.n_quads) return 1;
  if (w.ds.medium) { if (w.ds.motion) sim_aovs<true, true>(*sc, w, n, out); else sim_aovs<false, true>(*sc, w, n, out); }
  else { if (w.ds.motion) sim_aovs<true, false>(*sc, w, n, out); else sim_aovs<false, false>(*sc, w, n, out); }
  return 0;
}

// The surface record of every pixel: ids, kinds (height x width u32), ts (f64).
extern "C" int quad_sim_surface(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t* ids, uint32_t* kinds, double* ts) {
  World w;
  if (build(sc, center1, quads, n_quads, w) || !w.ds.n_quads) return 1;
  if (w.ds.medium) { if (w.ds.motion) sim_surface<true, true>(*sc, w, ids, kinds, ts); else sim_surface<false, true>(*sc, w, ids, kinds, ts); }
  else { if (w.ds.motion) sim_surface<true, false>(*sc, w, ids, kinds, ts); else sim_surface<false, false>(*sc, w, ids, kinds, ts); }
  return 0;
}
