// lane_sim.cpp — TEST TOOL, not part of the product.  The extern "C" surface of tests/lanesim/lane_sim.h (tests/lane_sim.py builds and
// binds it), and the per-feature probes: rt_neg_log, rt_solid.h and rt_quad.h built for the host, and the tables rt_tables.h builds.
#include <string>
#include <vector>

#include "lane_sim.h"

using namespace lanesim;

static_assert(sizeof(SurfRec) == 16, "the surface record is 16 bytes");

namespace {
// the loops by key: bits 0..2 = F_MEDIUM, F_SOLID, F_QUADS; bit 3 = HL for a frame, MOTION for the AOVs.  The surface record has no SOLID arm.
#define LANESIM_X16(F) {F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), F(8), F(9), F(10), F(11), F(12), F(13), F(14), F(15)}
#define LANESIM_RENDER(k) sim_render<((k) & 8) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, ((k) & F_QUADS) != 0>
#define LANESIM_AOVS(k) sim_aovs<((k) & 8) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, ((k) & F_QUADS) != 0>
#define LANESIM_SURFACE(k) sim_surface<((k) & 8) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_QUADS) != 0>
uint64_t (*const RENDER[16])(const RtScene&, const DevScene&, uint8_t*, float*) = LANESIM_X16(LANESIM_RENDER);
void (*const AOVS[16])(const RtScene&, const DevScene&, uint32_t, float*) = LANESIM_X16(LANESIM_AOVS);
void (*const SURFACE[16])(const RtScene&, const DevScene&, SurfRec*) = LANESIM_X16(LANESIM_SURFACE);  // (the F_SOLID entries repeat their neighbours)

// {grid n[0..2], n_large, n_items, wide}
void grid_info(const HostTables& t, uint32_t* info) {
  for (int k = 0; k < 3; ++k) info[k] = t.grid.n[k];
  info[3] = t.grid.n_large; info[4] = t.grid.n_items; info[5] = t.grid.wide;
}
template <typename V>
void put(std::vector<uint8_t>& blob, const V& v) {
  const uint64_t bytes = v.size() * sizeof(typename V::value_type);
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&bytes);
  blob.insert(blob.end(), p, p + 8);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(v.data());
  blob.insert(blob.end(), d, d + bytes);
}
}  // namespace

// ------------------------------------------------------------------ the lane code (each returns 1 when build_tables refused the world)
// The frame: rgb8 / linear (height x width x 3), segments traced.  Lit or unlit, static or moving; the arms by content | features_or.
extern "C" int lane_sim_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t features_or, uint8_t* rgb8,
                               float* linear, uint64_t* segments) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return 1;
  *segments = RENDER[(w.t.lights.empty() ? 0u : 8u) | ((features(w) | features_or) & 7u)](*sc, w.ds, rgb8, linear);
  return 0;
}

// The first-hit records of n samples per pixel (height x width x 8 f32).
extern "C" int lane_sim_aovs(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t features_or, uint32_t n, float* out) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return 1;
  AOVS[(w.ds.motion ? 8u : 0u) | ((features(w) | features_or) & 7u)](*sc, w.ds, n, out);
  return 0;
}

// The surface record of every pixel: out = height x width x {u32 id, u32 kind, f64 t}.
extern "C" int lane_sim_surface(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, void* out) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return 1;
  SURFACE[(w.ds.motion ? 8u : 0u) | features(w)](*sc, w.ds, static_cast<SurfRec*>(out));
  return 0;
}

// hit_world of n rays (lane_sim.h hit_rays).  tau: null = shutter time 0.  node: null = walk WITHOUT the medium candidate, even in a
// world that has media; a world without media walks as every other scene does.
extern "C" int lane_sim_hit_world_v(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* rays, const float* tau,
                                    const uint32_t* node, uint64_t n, int32_t* best, double* t, uint32_t* work) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return 1;
  const bool medium = node && w.ds.medium;
  if (w.ds.n_quads) (medium ? hit_rays<true, true> : hit_rays<false, true>)(*sc, w.ds, rays, tau, node, n, best, t, work);
  else (medium ? hit_rays<true, false> : hit_rays<false, false>)(*sc, w.ds, rays, tau, node, n, best, t, work);
  return 0;
}

// ------------------------------------------------------------------ the tables
// Every table build_tables fills, length-prefixed and back to back (geom, mat, matc, cell_word, cell_items, cell_items32, large, large_geom,
// motion, medium, lights, quads, then the GridDesc and the counts), into out (cap bytes).  Returns the blob's size, or -1 when build_tables
// refused the world; info = {n_solids, n_media, n_moving, wide, n_quads, simple_colour}.
extern "C" int64_t lane_sim_tables(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t* info, uint8_t* out, uint64_t cap) {
  World w;
  if (build(sc, center1, quads, n_quads, w)) return -1;
  const HostTables& t = w.t;
  info[0] = t.n_solids; info[1] = t.n_media; info[2] = t.n_moving; info[3] = t.grid.wide; info[4] = (uint32_t)t.quads.size(); info[5] = t.simple_colour;
  std::vector<uint8_t> blob;
  put(blob, t.geom); put(blob, t.mat); put(blob, t.matc); put(blob, t.cell_word); put(blob, t.cell_items); put(blob, t.cell_items32);
  put(blob, t.large); put(blob, t.large_geom); put(blob, t.motion); put(blob, t.medium); put(blob, t.lights); put(blob, t.quads);
  const uint8_t* g = reinterpret_cast<const uint8_t*>(&t.grid);
  blob.insert(blob.end(), g, g + sizeof t.grid);
  if (out && cap >= blob.size()) std::memcpy(out, blob.data(), blob.size());
  return (int64_t)blob.size();
}
// why build_tables refused the world ("" when it did not), into msg (cap bytes)
extern "C" void lane_sim_tables_error(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, char* msg, uint64_t cap) {
  HostTables t;
  const std::string why = build_tables(*sc, t, false, center1, quads, n_quads);
  std::strncpy(msg, why.c_str(), cap - 1);
  msg[cap - 1] = 0;
}

// The host's motion table (n x 4 {dv, pad}; pad 1 = moving) and its figures: info = {n_moving, grid n[0..2], n_large, n_items, wide}.
// Returns 0, 1 when build_tables refused the world, 2 when the table is empty (a static world: out untouched).
extern "C" int motion_table(const RtScene* sc, const double* center1, double* out, uint32_t* info) {
  World w;
  if (build(sc, center1, nullptr, 0, w)) return 1;
  info[0] = w.t.n_moving;
  grid_info(w.t, info + 1);
  if (w.t.motion.empty()) return 2;
  std::memcpy(out, w.t.motion.data(), w.t.motion.size() * sizeof(double));
  return 0;
}

// info = {n_media, grid n[0..2], n_large, n_items, wide}; listed[n_spheres] = number of cells that list sphere i (0 for a `large` one).
// Returns 0, or 1 when build_tables refused the world.
extern "C" int medium_tables(const RtScene* sc, const double* center1, uint32_t* info, uint32_t* listed, uint8_t* is_large) {
  World w;
  if (build(sc, center1, nullptr, 0, w)) return 1;
  info[0] = w.t.n_media;
  grid_info(w.t, info + 1);
  for (uint32_t i = 0; i < sc->n_spheres; ++i) { listed[i] = 0; is_large[i] = 0; }
  for (uint32_t i : w.t.large) is_large[i] = 1;
  if (w.t.grid.wide) for (uint32_t i : w.t.cell_items32) listed[i]++;
  else for (uint16_t i : w.t.cell_items) listed[i]++;
  return 0;
}

// Does the cell that holds the world-space point p[3] list sphere idx?  1 / 0; -1: the point lies outside the grid, the sphere is in
// the `large` list, or the world has no grid; -2: build_tables refused the world.
extern "C" int medium_cell_lists(const RtScene* sc, const double* p, uint32_t idx) {
  World w;
  if (build(sc, nullptr, nullptr, 0, w)) return -2;
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

// ------------------------------------------------------------------ rt_neg_log (csrc/common/rt_neg_log.h)
extern "C" void medium_neg_log_v(const double* x, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = rt_neg_log(x[i]);
}

// What medium_hit (rt_core.h) decides on, for tests/medium_rays.py to aim its rays with and to state its classes' conditions on: the
// functions medium_hit calls, in its order, for n (ray, sphere, density) triples.  rays = n x 6, spheres = n x 4 {centre, radius}, addr = n x 3
// {pixel, node, sphere index}.  out = n x 8: {disc, t1, t2, inside, u, dist, |d|^2 takes ray_consts' fast path (1 / 0), stage}, stage = 0: disc
// is not >= 0; 1: not t_in < t2; 2: not dist <= inside; 3: a candidate (t_in + dist / len).  The answer itself the tests take from
// hit_world, which calls medium_hit.
extern "C" void medium_terms_v(const double* rays, const double* spheres, const double* density, const uint32_t* addr, uint64_t seed, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; ++i) {
    const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    double* r = out + 8 * i;
    for (int k = 0; k < 8; ++k) r[k] = 0.0;
    const RayK rk = ray_consts(d);
    r[6] = rk.fast ? 1.0 : 0.0;
    const V3 oc = sub(o, v3(spheres[4 * i], spheres[4 * i + 1], spheres[4 * i + 2]));
    const double half_b = dot(oc, d);
    const double c = length_squared(oc) - spheres[4 * i + 3] * spheres[4 * i + 3];
    const double disc = (half_b * half_b) - (rk.a * c);
    r[0] = disc;
    if (!(disc >= 0.0)) continue;
    const double sq = rt_sqrt(disc);
    const double t1 = ((-half_b) - sq) / rk.a, t2 = ((-half_b) + sq) / rk.a;
    const double t_in = t1 > T_MIN ? t1 : T_MIN;
    r[1] = t1; r[2] = t2; r[7] = 1.0;
    if (!(t_in < t2)) continue;
    const double len = rt_sqrt(rk.a);
    const double inside = (t2 - t_in) * len;
    const U4 w = rng(RngAddr{addr[3 * i], 0u, (uint32_t)seed, (uint32_t)(seed >> 32)}, addr[3 * i + 1], MEDIUM_SLOT | addr[3 * i + 2]);
    const double u = u01_53(w.x, w.y);
    const double dist = rt_neg_log(1.0 - u) / density[i];
    r[3] = inside; r[4] = u; r[5] = dist; r[7] = 2.0;
    if (!(dist <= inside)) continue;
    r[7] = 3.0;
  }
}

// ------------------------------------------------------------------ rt_solid.h: p = n x 3 points already in the sphere's frame and scaled
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
  if (build(sc, nullptr, nullptr, 0, w)) return 1;
  const SphereGeom g = w.t.geom[idx];
  for (uint64_t i = 0; i < n; ++i) {
    const Rgb c = solid_albedo(v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), v3(g.cx, g.cy, g.cz), w.t.mat[idx]);
    colour[3 * i] = c.r; colour[3 * i + 1] = c.g; colour[3 * i + 2] = c.b;
  }
  return 0;
}

// ------------------------------------------------------------------ rt_quad.h
// rt_quad_prepare of n quads, quv = n x 9 (q, u, v): rec = n x 16 doubles (RtQuadRec), status[n] = its return value
extern "C" void quad_prepare_v(const double* quv, uint64_t n, double* rec, int32_t* status) {
  for (uint64_t i = 0; i < n; ++i) {
    RtQuadRec r;
    std::memset(&r, 0, sizeof r);
    status[i] = rt_quad_prepare(quv + 9 * i, quv + 9 * i + 3, quv + 9 * i + 6, &r);
    std::memcpy(rec + 16 * i, &r, sizeof r);
  }
}

// rt_quad_hit and rt_quad_normal of n rays (rays = n x 6: o, d) against ONE quad (quv = 9 doubles) with closest[n]:
// hit[n], t[n], P[n x 3], normal[n x 3], front[n] (zero where the ray does not hit).  Returns rt_quad_prepare's status.
extern "C" int quad_hit_v(const double* quv, const double* rays, const double* closest, uint64_t n, int32_t* hit, double* t, double* P, double* normal,
                          int32_t* front) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  for (uint64_t i = 0; i < n; ++i) {
    double tt = 0.0, pp[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
    const bool h = rt_quad_hit(r, rays + 6 * i, rays + 6 * i + 3, closest[i], &tt, pp);
    bool f = false;
    if (h) f = rt_quad_normal(r, rays + 6 * i + 3, nn);
    hit[i] = h; t[i] = h ? tt : 0.0; front[i] = f;
    for (int k = 0; k < 3; ++k) { P[3 * i + k] = h ? pp[k] : 0.0; normal[3 * i + k] = nn[k]; }
  }
  return 0;
}

// the six quads of a box, out = 6 x 9
extern "C" void quad_box(const double* mn, const double* mx, double* out) {
  double q[6][9];
  rt_box_quads(mn, mx, q);
  std::memcpy(out, q, sizeof q);
}
