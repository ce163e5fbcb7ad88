// tri_sim.cpp — TEST TOOL, not part of the product.  csrc/common/rt_quad.h's rt_flat_hit built for the host beside rt_quad_hit (the limit of
// DESIGN.md §21), and the limit table rt_tables.h builds; tests/tri_sim.py builds and binds it.  (The lane code itself — quads_hit with the
// limits behind the grid walk — is tests/lanesim/'s: DevScene::quads carries the limit table through its unchanged call.)
#include <cstdint>
#include <cstring>
#include <string>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"

using namespace rtc;

// rt_flat_hit and rt_quad_normal of n rays (rays = n x 6: o, d) against ONE flat primitive (quv = 9 doubles) of limit lim, with closest[n]:
// hit[n], t[n], P[n x 3], normal[n x 3], front[n] (zero where the ray does not hit).  Returns rt_quad_prepare's status.
extern "C" int flat_hit_v(const double* quv, double lim, const double* rays, const double* closest, uint64_t n, int32_t* hit, double* t, double* P,
                          double* normal, int32_t* front) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  for (uint64_t i = 0; i < n; ++i) {
    double tt = 0.0, pp[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
    const bool h = rt_flat_hit(r, lim, rays + 6 * i, rays + 6 * i + 3, closest[i], &tt, pp);
    bool f = false;
    if (h) f = rt_quad_normal(r, rays + 6 * i + 3, nn);
    hit[i] = h; t[i] = h ? tt : 0.0; front[i] = f;
    for (int k = 0; k < 3; ++k) { P[3 * i + k] = h ? pp[k] : 0.0; normal[3 * i + k] = nn[k]; }
  }
  return 0;
}

// rt_quad_hit, the same outputs (the test that lim = 2 is the old test wants both from one build)
extern "C" int quad_hit_v(const double* quv, const double* rays, const double* closest, uint64_t n, int32_t* hit, double* t, double* P) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  for (uint64_t i = 0; i < n; ++i) {
    double tt = 0.0, pp[3] = {0.0, 0.0, 0.0};
    const bool h = rt_quad_hit(r, rays + 6 * i, rays + 6 * i + 3, closest[i], &tt, pp);
    hit[i] = h; t[i] = h ? tt : 0.0;
    for (int k = 0; k < 3; ++k) P[3 * i + k] = h ? pp[k] : 0.0;
  }
  return 0;
}

// build_tables of the world: the limit table into lim (cap doubles) and info = {entries of quad_lim, n_tris, records, what bind_host_tables
// gave DevScene: lim non-null, n_tris}.  Returns 0, or 1 with build_tables' message in msg (cap_msg bytes).
extern "C" int tri_tables(const RtScene* sc, const RtQuad* quads, uint32_t n_quads, double* lim, uint64_t cap, uint32_t* info, char* msg, uint64_t cap_msg) {
  HostTables t;
  const std::string why = build_tables(*sc, t, false, nullptr, quads, n_quads);
  std::strncpy(msg, why.c_str(), cap_msg - 1);
  msg[cap_msg - 1] = 0;
  if (!why.empty()) return 1;
  DevScene ds;
  fill_dev_scene(*sc, t, ds);
  bind_host_tables(t, ds);
  info[0] = (uint32_t)t.quad_lim.size(); info[1] = t.n_tris; info[2] = (uint32_t)t.quads.size();
  info[3] = ds.quads.lim != nullptr; info[4] = ds.n_tris;
  for (uint64_t k = 0; k < t.quad_lim.size() && k < cap; ++k) lim[k] = t.quad_lim[k];
  return 0;
}
