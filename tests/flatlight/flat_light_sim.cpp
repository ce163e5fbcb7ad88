// flat_light_sim.cpp — TEST TOOL, not part of the product.  Flat primitives that emit built for the host: the header
// (csrc/common/rt_flat_light.h) on tables of words, and the lit QUADS lane code of tests/lanesim/lane_sim.h on a world bound as
// rt_hip_scene_set_flat_lights leaves it on the device — the emitters' material records of kind Light with the colour `emit`, the light list
// (Light spheres, then the emitters as object ids n_spheres + k), the light count and its thresholds, FLAT_LIGHTS_BIT.
// tests/flat_light_sim.py builds and binds it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"
// tests/lanesim/lane_sim.h — not to be edited — restates the kernels' QUADS arm with the call they made before the structure; in THIS build
// that call is the kernels' own (as in tests/flatmotion/flat_motion_sim.cpp)
#define quads_hit(o, d, view, n, base, closest, best) flats_hit(ds, tb, o, d, closest, best)
#include "../lanesim/lane_sim.h"
#undef quads_hit

using namespace lanesim;

namespace {
struct LitWorld {
  World w;
  std::vector<double> normals, still;
  std::vector<RtQuadRec> blob;
  std::vector<uint32_t> lights;
};
// info = {DevScene::n_tris, emitters, DevScene::n_lights}.  1: the world is refused; 2: a bad component (info[1] = the lowest entry); 3: bad normals
int build_lit(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const float* emit, int flat_bvh,
              LitWorld& s, uint32_t* info) {
  World& w = s.w;
  info[0] = info[1] = info[2] = 0;
  if (!sc || !n_quads || !build_tables(*sc, w.t, false, center1, quads, n_quads).empty()) return 1;
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
  if (smooth) {
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
    h->normals = s.normals.data(); w.ds.n_tris |= FLAT_NORMALS_BIT;
  }
  uint32_t n_emit = 0;
  if (emit) {
    const uint32_t bad = rt_flat_light_emit_check(emit, n_quads, &n_emit);
    if (bad != n_quads) { info[1] = bad; return 2; }
  }
  if (n_emit) {
    // the product's own table code (rt_tables.h build_flat_lights), bound as rt_hip_scene_set_flat_lights uploads it
    const std::vector<SphereMat> flat_mat(w.t.mat.begin() + sc->n_spheres, w.t.mat.end());
    const std::vector<MatCore> flat_matc(w.t.matc.begin() + sc->n_spheres, w.t.matc.end());
    std::vector<SphereMat> mat;
    std::vector<MatCore> matc;
    std::vector<uint32_t> emitters;
    build_flat_lights(flat_mat, flat_matc, w.t.lights, sc->n_spheres, emit, mat, matc, s.lights, emitters);
    std::copy(mat.begin(), mat.end(), w.t.mat.begin() + sc->n_spheres);
    std::copy(matc.begin(), matc.end(), w.t.matc.begin() + sc->n_spheres);
    w.ds.lights = s.lights.data();
    w.ds.n_lights = (uint32_t)s.lights.size();
    w.ds.light_thr[0] = 1.0 - (double)w.ds.n_lights * 0.1;
    w.ds.light_thr[1] = 1.0 - (double)w.ds.n_lights * 0.05;
    w.ds.n_tris |= FLAT_LIGHTS_BIT;
  }
  info[0] = w.ds.n_tris; info[1] = n_emit; info[2] = w.ds.n_lights;
  return 0;
}
#define FL_X8(F) {F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7)}
#define FL_RENDER(k) sim_render<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
#define FL_AOVS(k) sim_aovs<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
uint64_t (*const RENDER[8])(const RtScene&, const DevScene&, uint8_t*, float*) = FL_X8(FL_RENDER);   // bit 2: HL
void (*const AOVS[8])(const RtScene&, const DevScene&, uint32_t, float*) = FL_X8(FL_AOVS);          // bit 2: MOTION
// tests/lanesim/lane_sim.h's sim_render with the thin lens of DESIGN.md §13 (lane_begin_sample<true>: the camera ray leaves a point of the
// lens; DevScene::lens_u, lens_v, lens_r as rt_hip_set_lens leaves them): that loop is the pinhole camera's alone and is not to be edited
template <bool HL, bool MEDIUM, bool SOLID>
uint64_t lens_render(const RtScene& sc, const DevScene& ds, uint8_t* rgb8, float* linear) {
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
        lane_begin_sample<true>(ds, L, x, y);
        const float tau = ds.motion ? sample_time(L.ra) : 0.0f;
        for (;;) {
          L.n_segments++;
          const int st = with_tables(ds, tau, [&](const auto& tb) {
            double closest = T_MAX;
            int best = -1;
            uint32_t ns = 0;
            const MediumCtx mc{ds.medium, L.ra, L.node};
            hit_world_grid<MEDIUM>(ds, tb, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            const HitCB r = flats_hit(ds, tb, L.o, L.d, closest, best);
            return lane_shade<MEDIUM, SOLID, true>(ds, tb, L, r.best, r.closest);
          });
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
#define FL_LENS(k) lens_render<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0>
uint64_t (*const RENDER_LENS[8])(const RtScene&, const DevScene&, uint8_t*, float*) = FL_X8(FL_LENS);   // bit 2: HL
}  // namespace

// rt_flat_light_aim of n activations: quv[n][9], triangle[n], words[n][4] -> T[n][3]
extern "C" void fl_aim(const double* quv, const int32_t* triangle, const uint32_t* words, uint64_t n, double* T) {
  for (uint64_t i = 0; i < n; ++i) rt_flat_light_aim(quv + 9 * i, quv + 9 * i + 3, quv + 9 * i + 6, triangle[i] != 0, words + 4 * i, T + 3 * i);
}
// the (a, b) the words give BEFORE the fold, as the header's u01 makes them
extern "C" void fl_ab(const uint32_t* words, uint64_t n, double* ab) {
  for (uint64_t i = 0; i < n; ++i) { ab[2 * i] = rt_flat_light_u01(words[4 * i], words[4 * i + 1]); ab[2 * i + 1] = rt_flat_light_u01(words[4 * i + 2], words[4 * i + 3]); }
}
// the words of the aim draw of n activations {pixel, sample, node of the hit, light j}: rng(pixel, sample, child_node(node, j), RT_FLAT_LIGHT_SLOT)
extern "C" void fl_words(const uint32_t* act, uint64_t n, uint64_t seed, uint32_t* words) {
  for (uint64_t i = 0; i < n; ++i) {
    const RngAddr ra{act[4 * i], act[4 * i + 1], (uint32_t)seed, (uint32_t)(seed >> 32)};
    const U4 w = rng(ra, child_node(act[4 * i + 2], act[4 * i + 3]), RT_FLAT_LIGHT_SLOT);
    words[4 * i] = w.x; words[4 * i + 1] = w.y; words[4 * i + 2] = w.z; words[4 * i + 3] = w.w;
  }
}
extern "C" uint32_t fl_emit_check(const float* emit, uint32_t n, uint32_t* n_emitters) { return rt_flat_light_emit_check(emit, n, n_emitters); }

// The tables of the world as the kernels read them: mat / matc (all n_spheres + n_quads records; sizes[0], sizes[1]: their bytes) and the
// light list (sizes[2]: its count).  Any output may be null.
extern "C" int fl_tables(const RtScene* sc, const RtQuad* quads, uint32_t n_quads, const float* emit, void* mat, void* matc, uint32_t* lights, uint64_t* sizes,
                         uint32_t* info) {
  LitWorld s;
  if (const int rc = build_lit(sc, nullptr, quads, n_quads, nullptr, emit, 0, s, info)) return rc;
  const DevScene& d = s.w.ds;
  sizes[0] = s.w.t.mat.size() * sizeof(SphereMat); sizes[1] = s.w.t.matc.size() * sizeof(MatCore); sizes[2] = d.n_lights;
  if (mat) std::memcpy(mat, d.mat, sizes[0]);
  if (matc) std::memcpy(matc, d.matc, sizes[1]);
  if (lights && d.n_lights) std::memcpy(lights, d.lights, 4 * (size_t)d.n_lights);
  return 0;
}

// The frame of the QUADS lane code (lit where the world has a light).  normals: null or n x 9; emit: null or n x 3.
extern "C" int fl_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const float* emit, int flat_bvh,
                         uint8_t* rgb8, float* linear, uint64_t* segments, uint32_t* info) {
  LitWorld s;
  if (const int rc = build_lit(sc, center1, quads, n_quads, normals, emit, flat_bvh, s, info)) return rc;
  *segments = RENDER[(s.w.ds.n_lights ? 4u : 0u) | (features(s.w) & 3u)](*sc, s.w.ds, rgb8, linear);
  return 0;
}
// fl_render through a thin lens: lens = {u[3], v[3], radius}, the camera of `sc` already on the focus plane (rt_camera_derive_lens)
extern "C" int fl_render_lens(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const float* emit, int flat_bvh,
                              const double* lens, uint8_t* rgb8, float* linear, uint64_t* segments, uint32_t* info) {
  LitWorld s;
  if (const int rc = build_lit(sc, center1, quads, n_quads, normals, emit, flat_bvh, s, info)) return rc;
  for (int k = 0; k < 3; ++k) { s.w.ds.lens_u[k] = lens[k]; s.w.ds.lens_v[k] = lens[3 + k]; }
  s.w.ds.lens_r = lens[6];
  *segments = RENDER_LENS[(s.w.ds.n_lights ? 4u : 0u) | (features(s.w) & 3u)](*sc, s.w.ds, rgb8, linear);
  return 0;
}
// The first-hit records of n samples per pixel (height x width x 8 f32) and the surface record of every pixel (height x width x 16 B).
extern "C" int fl_aovs(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const float* emit, int flat_bvh,
                       uint32_t n, float* out, void* surface) {
  LitWorld s;
  uint32_t info[3];
  if (const int rc = build_lit(sc, center1, quads, n_quads, normals, emit, flat_bvh, s, info)) return rc;
  AOVS[(s.w.ds.motion ? 4u : 0u) | (features(s.w) & 3u)](*sc, s.w.ds, n, out);
  if (surface) {
    SurfRec* o = static_cast<SurfRec*>(surface);
    if (s.w.ds.motion) { if (s.w.ds.medium) sim_surface<true, true, true>(*sc, s.w.ds, o); else sim_surface<true, false, true>(*sc, s.w.ds, o); }
    else { if (s.w.ds.medium) sim_surface<false, true, true>(*sc, s.w.ds, o); else sim_surface<false, false, true>(*sc, s.w.ds, o); }
  }
  return 0;
}
