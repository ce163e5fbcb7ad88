// lane_smooth.cpp — TEST TOOL, not part of the product.  tests/lanesim/lane_sim.h's CPU build of the QUADS lane code (rt_core.h,
// rt_tables.h) with shading normals: the world as rt_hip_scene_set_flat_normals leaves it on the device — the 72-byte
// records of rt_flat_normal_prepare in entry order, their address in the FlatBvhHeader in front of the records (the structure's own header,
// or one of its own for a scan), FLAT_NORMALS_BIT in DevScene::n_tris — through sim_render and sim_aovs (tests/lane_smooth.py).
#include <vector>

#include "../lanesim/lane_sim.h"

using namespace lanesim;

namespace {
struct SmoothWorld {
  World w;
  std::vector<double> rec;          // [n_quads][9]
  std::vector<RtQuadRec> blob;      // a scan with normals: the header and the records behind it
};
// 0; 1: build_tables / build_flat_bvh refused the world; 2: a normal was refused (*bad_k = the lowest such entry)
int build_smooth(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, int flat_bvh, SmoothWorld& s,
                 uint32_t* bad_k) {
  World& w = s.w;
  if (!sc || !build_tables(*sc, w.t, false, center1, quads, n_quads).empty()) return 1;
  if (flat_bvh && !build_flat_bvh(w.t).empty()) return 1;
  fill_dev_scene(*sc, w.t, w.ds);
  bind_host_tables(w.t, w.ds);
  if (!normals) return 0;
  s.rec.assign(9 * (size_t)n_quads, 0.0);
  uint32_t count = 0;
  for (uint32_t k = 0; k < n_quads; ++k) {
    const int kind = rt_flat_normal_prepare(normals + 9 * (size_t)k, &s.rec[9 * (size_t)k]);
    const bool triangle = !w.t.quad_lim.empty() && w.t.quad_lim[k] == 1.0;
    if (kind == RT_FLAT_NORMAL_BAD || (kind == RT_FLAT_NORMAL_SMOOTH && !triangle)) { *bad_k = k; return 2; }
    count += kind == RT_FLAT_NORMAL_SMOOTH;
  }
  if (!count) return 0;           // no entry has normals: the scene is one that never had any
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
  h->normals = s.rec.data();
  w.ds.n_tris |= FLAT_NORMALS_BIT;
  return 0;
}
#define LANESIM_X8(F) {F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7)}
#define SMOOTH_RENDER(k) sim_render<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
#define SMOOTH_AOVS(k) sim_aovs<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
uint64_t (*const RENDER[8])(const RtScene&, const DevScene&, uint8_t*, float*) = LANESIM_X8(SMOOTH_RENDER);   // bit 2: HL
void (*const AOVS[8])(const RtScene&, const DevScene&, uint32_t, float*) = LANESIM_X8(SMOOTH_AOVS);          // bit 2: MOTION
}  // namespace

// The frame of the QUADS lane code.  normals: null, or n_quads x 9 as given to rt_hip_scene_set_flat_normals.  info = {DevScene::n_tris,
// entries whose record has normals, the lowest refused entry}.
extern "C" int lane_smooth_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, int flat_bvh,
                                  uint8_t* rgb8, float* linear, uint64_t* segments, uint32_t* info) {
  SmoothWorld s;
  info[0] = info[1] = 0; info[2] = 0xFFFFFFFFu;
  if (const int rc = build_smooth(sc, center1, quads, n_quads, normals, flat_bvh, s, info + 2)) return rc;
  if (!n_quads) return 1;
  info[0] = s.w.ds.n_tris;
  for (size_t k = 0; k < s.rec.size() / 9; ++k) info[1] += rt_flat_normal_present(&s.rec[9 * k]);
  const World& w = s.w;
  *segments = RENDER[(w.t.lights.empty() ? 0u : 4u) | (features(w) & 3u)](*sc, w.ds, rgb8, linear);
  return 0;
}

// The first-hit records of n samples per pixel (height x width x 8 f32).
extern "C" int lane_smooth_aovs(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, int flat_bvh, uint32_t n,
                                float* out) {
  SmoothWorld s;
  uint32_t bad = 0;
  if (const int rc = build_smooth(sc, center1, quads, n_quads, normals, flat_bvh, s, &bad)) return rc;
  if (!n_quads) return 1;
  AOVS[(s.w.ds.motion ? 4u : 0u) | (features(s.w) & 3u)](*sc, s.w.ds, n, out);
  return 0;
}
