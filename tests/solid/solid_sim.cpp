// CPU build of the solid textures (tests/test_solid_cpu.py; tests only): csrc/common/rt_solid.h built for the host, point by point, and
// the per-lane code of the SOLID kernels (rt_core.h scatter<MEDIUM, true> through lane_shade, aov_pixel's SOLID arm) one lane at a
// time on tables rt_tables.h built — what the SOLID megakernels and the SOLID rt_aov kernels run, without a GPU.
#include <cstdint>
#include <cstring>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"

using namespace rtc;

namespace {
struct World {
  HostTables t;
  DevScene ds;
};
int build(const RtScene* sc, const double* center1, World& w) {
  if (!build_tables(*sc, w.t, false, center1).empty()) return 1;
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
  return 0;
}
}  // namespace

// p = n x 3 points already in the sphere's frame and scaled
extern "C" void solid_checker_v(const double* p, uint64_t n, int32_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = rt_solid_checker_odd(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
extern "C" void solid_noise_v(const double* p, uint64_t n, uint32_t seed, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = rt_solid_noise(p[3 * i], p[3 * i + 1], p[3 * i + 2], seed);
}
extern "C" void solid_factor_v(const double* p, uint64_t n, uint32_t mode, uint32_t octaves, uint32_t seed, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = rt_solid_noise_factor(p[3 * i], p[3 * i + 1], p[3 * i + 2], mode, octaves, seed);
}

// solid_albedo of rt_core.h on the records rt_tables.h fills: colour[n x 3] of world-space hit points[n x 3] on sphere idx, the centre
// being the sphere's own.  Returns 1 when build_tables refused the world.
extern "C" int solid_albedo_v(const RtScene* sc, uint32_t idx, const double* points, uint64_t n, float* colour) {
  World w;
  if (build(sc, nullptr, w)) return 1;
  const SphereGeom g = w.t.geom[idx];
  for (uint64_t i = 0; i < n; ++i) {
    const Rgb c = solid_albedo(v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), v3(g.cx, g.cy, g.cz), w.t.mat[idx]);
    colour[3 * i] = c.r; colour[3 * i + 1] = c.g; colour[3 * i + 2] = c.b;
  }
  return 0;
}

// info = {n_solids, n_media, n_moving, wide}.  Returns 0, or 1 when build_tables refused the world.
extern "C" int solid_tables(const RtScene* sc, const double* center1, uint32_t* info) {
  World w;
  if (build(sc, center1, w)) return 1;
  info[0] = w.t.n_solids; info[1] = w.t.n_media; info[2] = w.t.n_moving; info[3] = w.t.grid.wide;
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
            st = lane_shade<MEDIUM, true>(ds, tb, L, best, closest);
          } else {
            hit_world_grid<MEDIUM>(ds, base, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            st = lane_shade<MEDIUM, true>(ds, base, L, best, closest);
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
    for (uint32_t x = 0; x < sc.width; ++x) aov_pixel<false, MOTION, MEDIUM, true>(w.ds, base, x, y, n, out + 8 * ((size_t)y * sc.width + x));
}
}  // namespace

// The pinhole camera; static or moving spheres; with or without media; lit or unlit.  -> rgb8 / linear (height x width x 3), segments.
extern "C" int solid_sim_render(const RtScene* sc, const double* center1, uint8_t* rgb8, float* linear, uint64_t* segments) {
  World w;
  if (build(sc, center1, w) || !w.t.n_solids) return 1;
  const bool hl = !w.t.lights.empty();
  if (w.ds.medium) *segments = hl ? sim_render<true, true>(*sc, w, rgb8, linear) : sim_render<false, true>(*sc, w, rgb8, linear);
  else *segments = hl ? sim_render<true, false>(*sc, w, rgb8, linear) : sim_render<false, false>(*sc, w, rgb8, linear);
  return 0;
}

// The first-hit records of n samples per pixel (height x width x 8 f32), the pinhole camera.
extern "C" int solid_sim_aovs(const RtScene* sc, const double* center1, uint32_t n, float* out) {
  World w;
  if (build(sc, center1, w) || !w.t.n_solids) return 1;
  if (w.ds.medium) { if (w.ds.motion) sim_aovs<true, true>(*sc, w, n, out); else sim_aovs<false, true>(*sc, w, n, out); }
  else { if (w.ds.motion) sim_aovs<true, false>(*sc, w, n, out); else sim_aovs<false, false>(*sc, w, n, out); }
  return 0;
}
