// CPU build of the tables and the per-lane grid walk with participating media (tests/test_medium_cpu.py; tests only).  rt_tables.h
// builds the tables of a world some of whose spheres are media (the density table, the grid that lists a medium in every cell its
// ball overlaps), and rt_core.h's hit_world_grid walks them with a MediumCtx — what the MEDIUM kernels do — at each ray's shutter time.
// Also rt_neg_log (csrc/common/rt_neg_log.h) built for the host.
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
  w.ds.cell_word = w.t.cell_word.data();
  w.ds.cell_items = w.t.grid.wide ? reinterpret_cast<const uint16_t*>(w.t.cell_items32.data()) : w.t.cell_items.data();
  w.ds.large = w.t.large.data();
  w.ds.large_geom = w.t.large_geom.data();
  w.ds.motion = w.t.motion.empty() ? nullptr : w.t.motion.data();
  w.ds.medium = w.t.medium.empty() ? nullptr : w.t.medium.data();
  return 0;
}
}  // namespace

extern "C" void medium_neg_log_v(const double* x, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = rt_neg_log(x[i]);
}

// info = {n_media, grid n[0..2], n_large, n_items, wide}; listed[n_spheres] = number of cells that list sphere i (0 for a `large` one).
// Returns 0, or 1 when build_tables refused the world.
extern "C" int medium_tables(const RtScene* sc, const double* center1, uint32_t* info, uint32_t* listed, uint8_t* is_large) {
  World w;
  if (build(sc, center1, w)) return 1;
  info[0] = w.t.n_media;
  for (int k = 0; k < 3; ++k) info[1 + k] = w.t.grid.n[k];
  info[4] = w.t.grid.n_large; info[5] = w.t.grid.n_items; info[6] = w.t.grid.wide;
  for (uint32_t i = 0; i < sc->n_spheres; ++i) { listed[i] = 0; is_large[i] = 0; }
  for (uint32_t i : w.t.large) is_large[i] = 1;
  if (w.t.grid.wide) for (uint32_t i : w.t.cell_items32) listed[i]++;
  else for (uint16_t i : w.t.cell_items) listed[i]++;
  return 0;
}

// hit_world_grid of n rays (n x 6 f64 {origin, direction}) at shutter times tau[n], ray i with the RNG address (pixel i, sample 0,
// node[i], the scene's seed) -> best[n], t[n], work[n x 2] = {exact tests, grid steps} (work may be null)
extern "C" int medium_hit_world_v(const RtScene* sc, const double* center1, const double* rays, const float* tau, const uint32_t* node,
                                  uint64_t n, int32_t* best, double* t, uint32_t* work) {
  World w;
  if (build(sc, center1, w)) return 1;
  const GlobalTables base{w.ds.geom, w.ds.matc};
  for (uint64_t i = 0; i < n; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    double closest = T_MAX;
    int b = -1;
    uint32_t ne = 0, ns = 0;
    MediumCtx mc;
    mc.density = w.ds.medium;
    mc.ra.pixel = (uint32_t)i; mc.ra.sample = 0; mc.ra.k0 = (uint32_t)sc->seed; mc.ra.k1 = (uint32_t)(sc->seed >> 32);
    mc.node = node[i];
    if (!w.ds.medium) {  // (a world without media: the walk every other scene gets)
      if (w.ds.motion) hit_world_grid(w.ds, motion_tables(base, w.ds.motion, tau[i]), o, d, closest, b, ne, ns);
      else hit_world_grid(w.ds, base, o, d, closest, b, ne, ns);
    } else if (w.ds.motion) hit_world_grid<true>(w.ds, motion_tables(base, w.ds.motion, tau[i]), o, d, closest, b, ne, ns, &mc);
    else hit_world_grid<true>(w.ds, base, o, d, closest, b, ne, ns, &mc);
    best[i] = b; t[i] = closest;
    if (work) { work[2 * i] = ne; work[2 * i + 1] = ns; }
  }
  return 0;
}

// Does the cell that holds the world-space point p[3] list sphere idx?  1 / 0; -1: the point lies outside the grid, the sphere is in
// the `large` list, or the world has no grid; -2: build_tables refused the world.
extern "C" int medium_cell_lists(const RtScene* sc, const double* p, uint32_t idx) {
  World w;
  if (build(sc, nullptr, w)) return -2;
  const GridDesc& G = w.t.grid;
  if (G.n[0] == 0u) return -1;
  for (uint32_t i : w.t.large) if (i == idx) return -1;
  uint32_t c[3];
  for (int k = 0; k < 3; ++k) {
    const double x = (p[k] - G.gmin[k]) * G.inv_cell[k];
    if (!(x >= 0.0 && x < (double)G.n[k])) return -1;
    c[k] = (uint32_t)x;
  }
  const uint32_t px = G.n[0] + 2, py = G.n[1] + 2;
  const size_t lin = (c[0] + 1) + (size_t)px * ((c[1] + 1) + (size_t)py * (c[2] + 1));
  const uint32_t first = G.wide ? w.t.cell_word[4 * lin] : (w.t.cell_word[2 * lin] & CELL_START_MASK);
  const uint32_t count = G.wide ? w.t.cell_word[4 * lin + 1] : (w.t.cell_word[2 * lin] >> CELL_COUNT_SHIFT);
  for (uint32_t k = 0; k < count; ++k)
    if ((G.wide ? w.t.cell_items32[first + k] : (uint32_t)w.t.cell_items[first + k]) == idx) return 1;
  return 0;
}

// The per-lane code of the MEDIUM kernels on the CPU, one lane at a time: lane_begin_sample, hit_world_grid<true> with the lane's RNG
// address, lane_shade<true> (scatter's medium arm), the pixel sums in exact fixed point as the kernels keep them.  Static or moving
// spheres, the pinhole camera.  -> rgb8 / linear (height x width x 3), segments traced.
namespace {
template <bool HL>
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
            hit_world_grid<true>(ds, tb, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            st = lane_shade<true>(ds, tb, L, best, closest);
          } else {
            hit_world_grid<true>(ds, base, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            st = lane_shade<true>(ds, base, L, best, closest);
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
}  // namespace

extern "C" int medium_sim_render(const RtScene* sc, const double* center1, uint8_t* rgb8, float* linear, uint64_t* segments) {
  World w;
  if (build(sc, center1, w) || !w.ds.medium) return 1;
  w.ds.mat = w.t.mat.data();
  w.ds.lights = w.t.lights.data();
  *segments = w.t.lights.empty() ? sim_render<false>(*sc, w, rgb8, linear) : sim_render<true>(*sc, w, rgb8, linear);
  return 0;
}
