// bvh_estimate.cpp — development analysis (not product; round 6): would a BVH over the spheres beat the single uniform grid + `large`
// list on worlds whose radii span decades ("a hierarchy remains unbuilt")?  Same rays as levels_estimate.cpp
// (a pinhole camera like scenes/procedural.py's, up to five diffuse bounces); the grid side is the PRODUCT's walk (hit_world_grid);
// the BVH: median split of the centroids' longest axis, leaves of <= 2 spheres, near child first, subtrees beyond `closest`
// skipped; every closest hit compared.  Counted per ray: grid = cell steps + exact tests; BVH = box tests + exact tests.  And the
// lock-step proxy that decides on a 64-wide wave: the MAX over 64 consecutive rays of those sums (a wave runs its slowest lane).
//   g++ -O2 -std=c++17 -ffp-contract=off -mfma -Iinclude tools/analysis/bvh_estimate.cpp -o /tmp/bvh;  /tmp/bvh world.bin
#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"
#include <random>
using namespace rtc;
struct Node { double lo[3], hi[3]; int left, right, first, count; };
static std::vector<Node> nodes; static std::vector<uint32_t> order; static const RtSphere* SP;
static void bounds(int a, int b, double lo[3], double hi[3]) {
  for (int k = 0; k < 3; ++k) { lo[k] = 1e300; hi[k] = -1e300; }
  for (int i = a; i < b; ++i) { const RtSphere& s = SP[order[i]]; const double r = fabs(s.radius);
    for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], s.center[k] - r); hi[k] = std::max(hi[k], s.center[k] + r); } }
}
static int build(int a, int b) {
  Node n; bounds(a, b, n.lo, n.hi); n.left = n.right = -1; n.first = a; n.count = b - a;
  const int id = (int)nodes.size(); nodes.push_back(n);
  if (b - a <= 2) return id;
  double clo[3] = {1e300, 1e300, 1e300}, chi[3] = {-1e300, -1e300, -1e300};
  for (int i = a; i < b; ++i) for (int k = 0; k < 3; ++k) { clo[k] = std::min(clo[k], SP[order[i]].center[k]); chi[k] = std::max(chi[k], SP[order[i]].center[k]); }
  int ax = 0; for (int k = 1; k < 3; ++k) if (chi[k] - clo[k] > chi[ax] - clo[ax]) ax = k;
  const int mid = (a + b) / 2;
  std::nth_element(order.begin() + a, order.begin() + mid, order.begin() + b, [&](uint32_t x, uint32_t y) { return SP[x].center[ax] < SP[y].center[ax]; });
  const int l = build(a, mid), r = build(mid, b);
  nodes[id].left = l; nodes[id].right = r; nodes[id].count = 0;
  return id;
}
static bool slab(const Node& n, V3 o, V3 inv, double tmax, double& tn) {
  double t0 = 0.001, t1 = tmax; const double oo[3] = {o.x, o.y, o.z}, ii[3] = {inv.x, inv.y, inv.z};
  for (int k = 0; k < 3; ++k) { double a = (n.lo[k] - oo[k]) * ii[k], b = (n.hi[k] - oo[k]) * ii[k]; if (a > b) std::swap(a, b); t0 = std::max(t0, a); t1 = std::min(t1, b); }
  tn = t0; return t0 <= t1;
}
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: bvh_estimate world.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); std::vector<double> raw; double b[4]; while (fread(b, 8, 4, f) == 4) raw.insert(raw.end(), b, b + 4); fclose(f);
  const size_t n = raw.size() / 4;
  std::vector<RtSphere> all(n); memset(all.data(), 0, sizeof(RtSphere) * n);
  for (size_t i = 0; i < n; i++) { all[i].center[0] = raw[4 * i]; all[i].center[1] = raw[4 * i + 1]; all[i].center[2] = raw[4 * i + 2]; all[i].radius = raw[4 * i + 3]; }
  RtScene sc; memset(&sc, 0, sizeof sc); sc.abi_version = RT_ABI_VERSION; sc.width = sc.height = 16; sc.samples_per_pixel = 1; sc.max_depth = 5; sc.n_spheres = (uint32_t)n; sc.spheres = all.data();
  HostTables t; build_tables(sc, t); DevScene ds; fill_dev_scene(sc, t, ds);
  if (t.grid.wide) { fprintf(stderr, "wide grid: not handled here\n"); return 2; }
  bind_host_tables(t, ds);
  printf("grid %ux%ux%u items %u large %u | ", t.grid.n[0], t.grid.n[1], t.grid.n[2], t.grid.n_items, t.grid.n_large);
  // the BVH holds every sphere but the ground (r >= 100: tested by every ray, like the grid's `large` list does)
  SP = all.data(); std::vector<uint32_t> always;
  for (size_t i = 0; i < n; i++) if (fabs(all[i].radius) >= 100) always.push_back((uint32_t)i); else order.push_back((uint32_t)i);
  build(0, (int)order.size());
  printf("bvh %zu nodes over %zu spheres (+%zu always tested)\n", nodes.size(), order.size(), always.size());
  std::mt19937_64 g(7); std::uniform_real_distribution<double> U(-1, 1);
  auto rnd_unit = [&]() { for (;;) { V3 p = v3(U(g), U(g), U(g)); double l = length_squared(p); if (l < 1 && l > 1e-6) return muls(p, 1 / sqrt(l)); } };
  double gT = 0, gS = 0, bT = 0, bB = 0; long rays = 0, mism = 0; double gmax = 0, bmax = 0; long groups = 0; uint32_t cur_g = 0, cur_b = 0; int in_group = 0;
  V3 cam = v3(13, 2, 3), fwd = unit_vector(sub(v3(0, 0, 0), cam)); V3 right = unit_vector(v3(fwd.z, 0, -fwd.x));
  V3 up = v3(right.y * fwd.z - right.z * fwd.y, right.z * fwd.x - right.x * fwd.z, right.x * fwd.y - right.y * fwd.x);
  const double th = tan(10.0 * M_PI / 180.0);
  std::vector<int> stack;
  for (int s = 0; s < 300000; s++) {
    V3 o = cam; V3 d = add(fwd, add(muls(right, U(g) * th * 16.0 / 9.0), muls(up, U(g) * th)));
    for (int depth = 0; depth < 6; depth++) {
      double c1 = T_MAX; int b1 = -1; uint32_t ne = 0, ns = 0; const GlobalTables tb{ds.geom, ds.matc}; hit_world_grid(ds, tb, o, d, c1, b1, ne, ns);
      double c2 = T_MAX; int b2 = -1; uint32_t me = 0, mb = 0; const RayK a = ray_consts(d); const V3 inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
      for (uint32_t i : always) { SphereGeom gg{all[i].center[0], all[i].center[1], all[i].center[2], all[i].radius}; me++; int bb = b2; if (exact_hit_any_order(o, d, a, gg, i, c2, bb)) b2 = bb; }
      stack.clear(); stack.push_back(0);
      while (!stack.empty()) {
        const int id = stack.back(); stack.pop_back(); const Node& nd = nodes[id]; double tn; mb++;
        if (!slab(nd, o, inv, c2, tn)) continue;
        if (nd.left < 0) { for (int k = 0; k < nd.count; ++k) { const uint32_t i = order[nd.first + k]; SphereGeom gg{all[i].center[0], all[i].center[1], all[i].center[2], all[i].radius}; me++; int bb = b2; if (exact_hit_any_order(o, d, a, gg, i, c2, bb)) b2 = bb; } continue; }
        double tl, tr; const bool hl = slab(nodes[nd.left], o, inv, c2, tl), hr = slab(nodes[nd.right], o, inv, c2, tr);   // (peek: near child first; the children's own tests are counted when popped)
        if (hl && hr) { if (tl <= tr) { stack.push_back(nd.right); stack.push_back(nd.left); } else { stack.push_back(nd.left); stack.push_back(nd.right); } }
        else if (hl) stack.push_back(nd.left); else if (hr) stack.push_back(nd.right);
      }
      gT += ne; gS += ns; bT += me; bB += mb; rays++;
      if (b1 != b2 || (b1 >= 0 && c1 != c2)) mism++;
      cur_g = std::max(cur_g, ne + ns); cur_b = std::max(cur_b, me + mb);
      if (++in_group == 64) { gmax += cur_g; bmax += cur_b; groups++; cur_g = cur_b = 0; in_group = 0; }
      if (b1 < 0) break;
      V3 p = add(o, muls(d, c1)); const RtSphere& sp = all[b1]; V3 nrm = muls(sub(p, v3(sp.center[0], sp.center[1], sp.center[2])), 1.0 / sp.radius); if (dot(nrm, d) > 0) nrm = neg(nrm);
      o = p; d = add(nrm, rnd_unit());
    }
  }
  printf("rays %ld mismatches %ld | grid: %.2f tests + %.2f steps per ray, max over 64 consecutive rays %.1f | bvh: %.2f tests + %.2f box tests per ray, max over 64 %.1f\n",
         rays, mism, gT / rays, gS / rays, gmax / groups, bT / rays, bB / rays, bmax / groups);
  return 0;
}
