// lane_sim.h — TEST TOOL, not part of the product.  The per-lane code of rt_core.h built for the CPU and driven one lane at a time on
// tables rt_tables.h built on the host: what the megakernels, rt_aov* and rt_surface* run, without a GPU.  One World, one ray-batch
// walk, one copy each of the frame, AOV and surface loops; tests/lanesim/lane_sim.cpp exports them and tests/lane_sim.py binds them.
//
// Which instantiation runs.  Every loop is a template over the product's feature arms and is picked from a table by the scene's
// content, by the rule of select_kernel (rt_hip_api.hip): HL = the scene has lights, MEDIUM = a density table (ds.medium), SOLID =
// t.n_solids != 0, QUADS = ds.n_quads != 0, MOTION = a motion table (ds.motion).  So a caller gets the instantiation the GPU launches
// for that scene.  The frame and AOV entry points take a `features_or` mask that is ORed into that key, for a test that wants an arm
// its scene does not ask for: tests/test_quad_cpu.py passes F_SOLID, as its simulator always ran lane_shade<MEDIUM, true, true>;
// every other caller passes 0.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"

namespace lanesim {
using namespace rtc;

enum : uint32_t { F_MEDIUM = 1, F_SOLID = 2, F_QUADS = 4 };  // the feature bits of a key and of `features_or`

struct World {
  HostTables t;
  DevScene ds;
};
// center1: null, or the centres at shutter close; quads: null / 0 for a scene without one.  Returns 1 when build_tables refused the world.
inline int build(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, World& w) {
  if (!sc || !build_tables(*sc, w.t, false, center1, quads, n_quads).empty()) return 1;
  fill_dev_scene(*sc, w.t, w.ds);
  bind_host_tables(w.t, w.ds);
  return 0;
}
inline uint32_t features(const World& w) { return (w.ds.medium ? F_MEDIUM : 0u) | (w.t.n_solids ? F_SOLID : 0u) | (w.ds.n_quads ? F_QUADS : 0u); }

// f(tables) with the tables the kernels read: the motion tables at shutter time tau in a world that moves, the resident ones otherwise
template <class F>
auto with_tables(const DevScene& ds, float tau, F&& f) {
  const GlobalTables base{ds.geom, ds.matc};
  return ds.motion ? f(motion_tables(base, ds.motion, tau)) : f(base);
}

// hit_world of the kernels for one ray: the grid walk (with the medium candidate of RNG address `ra`, `node` when MEDIUM), then the quads
template <bool MEDIUM, bool QUADS, class Tables>
void hit_world(const DevScene& ds, const Tables& tb, V3 o, V3 d, const RngAddr& ra, uint32_t node, double& closest, int& best, uint32_t& n_exact,
               uint32_t& n_steps) {
  const MediumCtx mc{ds.medium, ra, node};
  hit_world_grid<MEDIUM>(ds, tb, o, d, closest, best, n_exact, n_steps, &mc);
  if constexpr (QUADS) {
    const HitCB r = quads_hit(o, d, ds.quads, ds.n_quads, ds.n_spheres, closest, best);
    closest = r.closest; best = r.best;
  }
}

// n rays (n x 6 f64 {origin, direction}) at shutter times tau[n] (null: 0), ray i with the RNG address (pixel i, sample 0, node[i], the
// scene's seed) -> best[n] (object id, -1: a miss), t[n] (`closest` as the walk left it), work[n x 2] = {exact tests, grid steps} (or null)
template <bool MEDIUM, bool QUADS>
void hit_rays(const RtScene& sc, const DevScene& ds, const double* rays, const float* tau, const uint32_t* node, uint64_t n, int32_t* best, double* t,
              uint32_t* work) {
  for (uint64_t i = 0; i < n; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const RngAddr ra{(uint32_t)i, 0u, (uint32_t)sc.seed, (uint32_t)(sc.seed >> 32)};
    double closest = T_MAX;
    int b = -1;
    uint32_t ne = 0, ns = 0;
    with_tables(ds, tau ? tau[i] : 0.0f, [&](const auto& tb) { hit_world<MEDIUM, QUADS>(ds, tb, o, d, ra, MEDIUM ? node[i] : 0u, closest, b, ne, ns); });
    best[i] = b; t[i] = closest;
    if (work) { work[2 * i] = ne; work[2 * i + 1] = ns; }
  }
}

// The megakernel's lane: lane_begin_sample, hit_world with the lane's RNG address, lane_shade, the pixel sums in exact fixed point as the
// kernels keep them.  The pinhole camera.  -> rgb8 / linear (height x width x 3); returns the segments traced.
template <bool HL, bool MEDIUM, bool SOLID, bool QUADS>
uint64_t sim_render(const RtScene& sc, const DevScene& ds, uint8_t* rgb8, float* linear) {
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
          L.n_segments++;
          const int st = with_tables(ds, tau, [&](const auto& tb) {
            double closest = T_MAX;
            int best = -1;
            uint32_t ns = 0;
            hit_world<MEDIUM, QUADS>(ds, tb, L.o, L.d, L.ra, L.node, closest, best, L.n_exact, ns);
            return lane_shade<MEDIUM, SOLID, QUADS>(ds, tb, L, best, closest);
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

// The first-hit records of n samples per pixel (height x width x 8 f32), the pinhole camera (LENS false).
template <bool MOTION, bool MEDIUM, bool SOLID, bool QUADS>
void sim_aovs(const RtScene& sc, const DevScene& ds, uint32_t n, float* out) {
  const GlobalTables base{ds.geom, ds.matc};
  for (uint32_t y = 0; y < sc.height; ++y)
    for (uint32_t x = 0; x < sc.width; ++x) aov_pixel<false, MOTION, MEDIUM, SOLID, QUADS>(ds, base, x, y, n, out + 8 * ((size_t)y * sc.width + x));
}

// The surface record of every pixel, height x width.
template <bool MOTION, bool MEDIUM, bool QUADS>
void sim_surface(const RtScene& sc, const DevScene& ds, SurfRec* out) {
  const GlobalTables base{ds.geom, ds.matc};
  for (uint32_t y = 0; y < sc.height; ++y)
    for (uint32_t x = 0; x < sc.width; ++x) out[(size_t)y * sc.width + x] = surface_pixel<MOTION, MEDIUM, QUADS>(ds, base, x, y);
}

}  // namespace lanesim
