// update_harness.cpp — TEST INFRASTRUCTURE (tests/test_update_cpu.py): digests of the tables rt_tables.h builds for a scene, and the
// CLI's per-frame centres (csrc/host/anim_path.h), behind a C interface.
#include <cstdint>
#include <cstring>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"
#include "../../rust-raytracer_amd/csrc/host/anim_path.h"

namespace {
uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
template <typename V> uint64_t fnv_vec(const V& v) { return fnv(v.data(), v.size() * sizeof(typename V::value_type)) ^ (uint64_t)v.size(); }
}  // namespace

// out[0..7] = grid, cell_word, cell_items (packed or wide), large, large_geom, geom, motion, n_moving; returns 0, or 1 for an invalid scene
extern "C" int update_tables_digest(const RtScene* sc, const double* center1, uint64_t out[8]) {
  rtc::HostTables t;
  if (!rtc::build_tables(*sc, t, false, center1).empty()) return 1;
  out[0] = fnv(&t.grid, sizeof t.grid);
  out[1] = fnv_vec(t.cell_word);
  out[2] = t.grid.wide ? fnv_vec(t.cell_items32) : fnv_vec(t.cell_items);
  out[3] = fnv_vec(t.large);
  out[4] = fnv_vec(t.large_geom);
  out[5] = fnv_vec(t.geom);
  out[6] = fnv_vec(t.motion);
  out[7] = t.n_moving;
  return 0;
}

extern "C" void update_anim_centres(const RtSphere* spheres, const double* center1, uint32_t n, int f, int N, double S, double* c_out, double* c1_out) {
  rt_anim_centres(spheres, center1, n, f, N, S, c_out, c1_out);
}
