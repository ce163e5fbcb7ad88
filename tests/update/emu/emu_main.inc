// TEST INFRASTRUCTURE: the device grid build (emulated, see hip/hip_runtime.h) against the host builder on a few worlds, byte for byte.
// Pasted behind the kernels of rt_grid_build.hip by tests/test_update_cpu.py.
#include <random>
#include <cstdio>
using namespace rtc;
static int run(const char* what, std::vector<RtSphere> sp, const std::vector<double>* c1, bool force_wide) {
  RtScene sc{}; sc.abi_version = RT_ABI_VERSION; sc.width = 4; sc.height = 4; sc.spheres = sp.data(); sc.n_spheres = (uint32_t)sp.size();
  if (force_wide) setenv("RT_GRID_WIDE", "1", 1); else unsetenv("RT_GRID_WIDE");
  HostTables ref;
  std::string why = build_tables(sc, ref, false, c1 ? c1->data() : nullptr);
  if (!why.empty()) { std::printf("%s: invalid %s\n", what, why.c_str()); return 1; }
  // the update path
  const uint32_t n = sc.n_spheres;
  HostTables t; build_motion(sc, c1 ? c1->data() : nullptr, t);
  GridParams gp = grid_params_shipped();
  const bool want_wide = gp.force_wide || n > 65535u;
  rtgb::Job j; GridPlan plan;
  j.all_large = grid_plan(sc, t, gp, want_wide, j.G, plan) != GRID_PLAN_GRID;
  if (j.all_large) std::memset(&j.G, 0, sizeof j.G);
  const uint32_t inner = j.all_large ? 0u : rtgb::inner_cells(j.G);
  std::vector<double> centre(3 * (size_t)n); std::vector<SphereGeom> old_geom(n), geom(n);
  for (uint32_t i = 0; i < n; ++i) { for (int k = 0; k < 3; ++k) centre[3 * i + k] = sp[i].center[k]; old_geom[i] = SphereGeom{1e9, -1e9, 7.0, sp[i].radius}; }
  std::vector<GridRange> range(n); std::vector<uint32_t> lflag(n), lpos(n), count(inner + 1), start(inner + 1), cursor(inner + 1);
  std::vector<unsigned long long> bsum(rtgb::scan_blocks(std::max<size_t>(n, inner)) + 1);
  rtgb::Counts cnt{};
  j.n = n; for (int k = 0; k < 3; ++k) j.cell_w[k] = plan.cell_w[k]; j.m = plan.m; j.large_cell_limit = gp.large_cell_limit;
  j.centre = centre.data(); j.old_geom = old_geom.data(); j.motion = t.n_moving ? t.motion.data() : nullptr; j.plan_large = plan.is_large.data();
  j.range = range.data(); j.lflag = lflag.data(); j.lpos = lpos.data(); j.count = count.data(); j.start = start.data(); j.cursor = cursor.data();
  j.block_sum = bsum.data(); j.counts = &cnt; j.geom = geom.data();
  rtgb::count(j, nullptr);
  bool wide = want_wide;
  if (!j.all_large && !wide && (cnt.max_count > CELL_MAX_COUNT || cnt.n_items >= CELL_START_MASK)) wide = true;
  j.G.n_items = (uint32_t)cnt.n_items; j.G.n_large = (uint32_t)cnt.n_large; j.G.wide = (!j.all_large && wide) ? 1u : 0u;
  std::vector<uint32_t> cell_word((size_t)j.G.n_cells * (j.G.wide ? 4 : 2) + 4, 0xABABABABu), raw_items(j.G.n_items + 1), raw_cell(j.G.n_items + 1), large(j.G.n_large + 1);
  std::vector<uint8_t> items((size_t)j.G.n_items * (j.G.wide ? 4 : 2) + 8, 0xCD);
  std::vector<SphereGeom> large_geom(j.G.n_large + 1);
  j.raw_items = raw_items.data(); j.raw_cell = raw_cell.data(); j.cell_word = cell_word.data(); j.cell_items = items.data(); j.large = large.data(); j.large_geom = large_geom.data();
  rtgb::tables(j, cnt.n_items, cnt.n_large, j.G.wide != 0, nullptr);
  int bad = 0;
  auto cmp = [&](const char* name, const void* a, const void* b, size_t bytes) { if (bytes && std::memcmp(a, b, bytes)) { std::printf("%s: %s differs\n", what, name); bad++; } };
  cmp("grid", &j.G, &ref.grid, sizeof j.G);
  if (!bad) {
    cmp("cell_word", cell_word.data(), ref.cell_word.data(), ref.cell_word.size() * 4);
    if (ref.grid.wide) cmp("items32", items.data(), ref.cell_items32.data(), ref.cell_items32.size() * 4); else cmp("items16", items.data(), ref.cell_items.data(), ref.cell_items.size() * 2);
    cmp("large", large.data(), ref.large.data(), ref.large.size() * 4);
    cmp("large_geom", large_geom.data(), ref.large_geom.data(), ref.large_geom.size() * sizeof(SphereGeom));
    cmp("geom", geom.data(), ref.geom.data(), n * sizeof(SphereGeom));
  }
  std::printf("%s: n %u cells %u items %u large %u wide %u moving %u max_count %u -> %s\n", what, n, ref.grid.n_cells, ref.grid.n_items, ref.grid.n_large, ref.grid.wide, t.n_moving, cnt.max_count, bad ? "DIFFERENT" : "equal");
  return bad;
}
int main() {
  std::mt19937_64 rng(7); std::uniform_real_distribution<double> U(0.0, 1.0);
  auto sph = [](double x, double y, double z, double r) { RtSphere s{}; s.center[0] = x; s.center[1] = y; s.center[2] = z; s.radius = r; return s; };
  int bad = 0;
  { std::vector<RtSphere> v{sph(0, -1000, 0, 1000), sph(0, 1, 0, 1), sph(-4, 1, 0, 1), sph(4, 1, 0, -1)};
    for (int a = -11; a < 11; ++a) for (int b = -11; b < 11; ++b) v.push_back(sph(a + 0.9 * U(rng), 0.2, b + 0.9 * U(rng), 0.2));
    bad += run("lattice488", v, nullptr, false);
    std::vector<double> c1; for (auto& s : v) for (int k = 0; k < 3; ++k) c1.push_back(s.center[k]);
    for (size_t i = 4; i < v.size(); i += 3) { c1[3 * i] += 0.3 * U(rng); c1[3 * i + 1] += 0.2 * U(rng); } c1[3 * 2 + 1] += 0.4;
    bad += run("moving", v, &c1, false);
    bad += run("lattice wide", v, nullptr, true);
    v[9].center[1] = NAN; bad += run("one nan", v, nullptr, false); }
  { std::vector<RtSphere> v; for (int i = 0; i < 3000; ++i) v.push_back(sph(20 * U(rng), 3 * U(rng), 20 * U(rng), 0.05 + 0.3 * U(rng)));
    bad += run("random3000", v, nullptr, false); }
  { std::vector<RtSphere> v; for (int i = 0; i < 23; ++i) v.push_back(sph(U(rng), U(rng), U(rng), 0.1)); bad += run("23", v, nullptr, false);
    v.push_back(sph(0.5, 0.5, 0.5, 0.1)); v.push_back(sph(0.1, 0.5, 0.5, 0.1)); bad += run("25", v, nullptr, false); }
  { std::vector<RtSphere> v{sph(0, -1000, 0, 1000)}; for (int i = 0; i < 5000; ++i) v.push_back(sph(0.5, 0.02, 0.5, 0.02));
    for (int i = 0; i < 300; ++i) v.push_back(sph(16 * U(rng) - 8, 0.02, 16 * U(rng) - 8, 0.02)); bad += run("crowd5000", v, nullptr, false); }
  { std::vector<RtSphere> v; for (int a = -10; a < 10; ++a) for (int b = -10; b < 10; ++b) v.push_back(sph(0.05 * (a + 0.5), 0.1, 0.05 * (b + 0.5), 0.1));
    v.push_back(sph(0, 0.39, 0, 0.39)); bad += run("demote", v, nullptr, false); }
  std::printf(bad ? "FAILED\n" : "ALL EQUAL\n");
  return bad;
}
