// CPU build of the motion-blur tables and the per-lane grid walk (tests/test_motion.py; tests only).  rt_tables.h builds the tables
// of a world whose spheres move from center to center1 (build_tables' center1: swept-box listing, the dv table), and rt_core.h's
// hit_world_grid walks them through MotionTables — the accessor the MOTION kernels use — at each ray's shutter time tau.
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
  return 0;
}
}  // namespace

// The host's motion table (n x 4 {dv, pad}; pad 1 = moving) and its figures: info = {n_moving, grid n[0..2], n_large, n_items, wide}.
// Returns 0, 1 when build_tables refused the world, 2 when the table is empty (a static world: out untouched).
extern "C" int motion_table(const RtScene* sc, const double* center1, double* out, uint32_t* info) {
  World w;
  if (build(sc, center1, w)) return 1;
  info[0] = w.t.n_moving;
  for (int k = 0; k < 3; ++k) info[1 + k] = w.t.grid.n[k];
  info[4] = w.t.grid.n_large; info[5] = w.t.grid.n_items; info[6] = w.t.grid.wide;
  if (w.t.motion.empty()) return 2;
  std::memcpy(out, w.t.motion.data(), w.t.motion.size() * sizeof(double));
  return 0;
}

// hit_world_grid of n rays (n x 6 f64 {origin, direction}) at shutter times tau[n] (f32, as the kernel keeps them) through the
// motion tables -> best[n], t[n], work[n x 2] = {exact tests, grid steps} (work may be null)
extern "C" int motion_hit_world_v(const RtScene* sc, const double* center1, const double* rays, const float* tau, uint64_t n,
                                  int32_t* best, double* t, uint32_t* work) {
  World w;
  if (build(sc, center1, w)) return 1;
  const GlobalTables base{w.ds.geom, w.ds.matc};
  for (uint64_t i = 0; i < n; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    double closest = T_MAX;
    int b = -1;
    uint32_t ne = 0, ns = 0;
    if (w.ds.motion) hit_world_grid(w.ds, motion_tables(base, w.ds.motion, tau[i]), o, d, closest, b, ne, ns);
    else hit_world_grid(w.ds, base, o, d, closest, b, ne, ns);
    best[i] = b; t[i] = closest;
    if (work) { work[2 * i] = ne; work[2 * i + 1] = ns; }
  }
  return 0;
}
