// rt_grid_build.h — the uniform grid's per-sphere and per-cell expressions, shared by the host builder (rt_tables.h build_grid_as:
// what rt_hip_scene_create* runs) and the device builder (rt_grid_build.hip: what rt_hip_scene_update_spheres runs), and the
// device builder's entry points.  Both sides compile these f64 expressions without contraction (-ffp-contract=off), every operation
// in them is correctly rounded or exact (+ - * floor fabs compare), so they give the same bits on both.
#pragma once
#include "rt_core.h"

namespace rtc {

// The box a sphere's centre can occupy over the shutter, one axis: [c0 - |r|, c0 + |r|] for a static sphere, and for a moving one the
// union of its boxes at c0 and c0 + dv, grown by a world-space slack that bounds the rounding of the kernel's c0 + dv * tau (two f64
// roundings, each <= 2^-53 of |c0| + |dv|) off the true segment: 4 * 2^-52 (|c0| + |dv|) + 1e-300.
RT_HD void grid_sphere_box(double c0, double radius, bool moves, double dv, double& lo, double& hi) {
  const double r = fabs(radius);
  if (!moves) { lo = c0 - r; hi = c0 + r; return; }
  const double c1 = c0 + dv;
  const double slack = 4.0 * 2.220446049250313e-16 * (fabs(c0) + fabs(dv)) + 1e-300;
  lo = (c1 < c0 ? c1 : c0) - r - slack;
  hi = (c0 < c1 ? c1 : c0) + r + slack;
}

// Cell range of a gridded sphere along each axis: its box grown by the registration margin m (in cells, 2 * GridDesc.pull), cut to
// the grid.  mv: its motion row {dv, moves} or null (static).  Returns the number of cells of the range (0: an empty one).
struct GridRange { int a[3], b[3]; };
RT_HD uint64_t grid_cell_range(const GridDesc& G, double m, const double c[3], double radius, const double* mv, GridRange& rg) {
  uint64_t cells = 1;
  const bool moves = mv && mv[3] != 0.0;
  for (int k = 0; k < 3; ++k) {
    double bl, bh;
    grid_sphere_box(c[k], radius, moves, moves ? mv[k] : 0.0, bl, bh);
    double a = floor((bl - G.gmin[k]) * G.inv_cell[k] - m);
    double b = floor((bh - G.gmin[k]) * G.inv_cell[k] + m);
    a = a < 0.0 ? 0.0 : a;
    b = G.nd[k] - 1.0 < b ? G.nd[k] - 1.0 : b;
    rg.a[k] = (int)a; rg.b[k] = (int)b;
    cells *= (uint64_t)(b >= a ? (int)b - (int)a + 1 : 0);
  }
  return cells;
}

// does the cell (grown by the margin) come within |r| of the centre?  (world units, f64; cell_w[k] = 1.0 / G.inv_cell[k])
RT_HD bool grid_overlaps(const GridDesc& G, const double cell_w[3], double m, const double c[3], double radius, int ix, int iy, int iz) {
  const int idx[3] = {ix, iy, iz};
  double d2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double w = cell_w[k];
    const double c0 = G.gmin[k] + ((double)idx[k] - m) * w, c1 = G.gmin[k] + ((double)idx[k] + 1.0 + m) * w;
    const double d = c[k] < c0 ? c0 - c[k] : (c[k] > c1 ? c[k] - c1 : 0.0);
    d2 += d * d;
  }
  const double r = fabs(radius) * (1.0 + 1e-9);
  return d2 <= r * r;
}

}  // namespace rtc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// The device builder: everything of the grid that is per (sphere, cell) or per cell.  Two phases around ONE small readback
// (Counts): count() up to the totals the host sizes the item buffers and picks the table format with, then tables().
// Every pointer is device memory; all work is enqueued on `stream`; a function returns the first HIP launch error.
namespace rtgb {

struct Counts {              // what count() leaves in Job::counts
  unsigned long long n_items;  // items of all cells
  unsigned long long n_large;  // spheres of the `large` list
  uint32_t max_count;          // items of the fullest cell
  uint32_t pad;
};
constexpr uint32_t SCAN_BLOCK = 256, SCAN_PER_THREAD = 8, SCAN_TILE = SCAN_BLOCK * SCAN_PER_THREAD;
inline size_t scan_blocks(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

struct Job {
  uint32_t n = 0;                      // spheres
  bool all_large = false;              // no grid: every sphere goes to the `large` list (G is all zero but n_large)
  rtc::GridDesc G{};                   // as the host planned it (n_items, n_large, wide are the host's to fill in after count())
  double cell_w[3] = {0, 0, 0};        // 1.0 / G.inv_cell[k], divided on the host
  double m = 0.0;                      // registration margin, cells
  uint32_t large_cell_limit = 0;
  // inputs
  const double* centre = nullptr;          // [n][3] the new centres
  const rtc::SphereGeom* old_geom = nullptr;  // [n] the radii come from here
  const double* motion = nullptr;          // [n][4] or null: a static scene
  const uint8_t* plan_large = nullptr;     // [n] 1: the host's plan put the sphere into `large` (non-finite, or by radius)
  // scratch
  rtc::GridRange* range = nullptr;         // [n]
  uint32_t* lflag = nullptr, * lpos = nullptr;  // [n] 1: in `large`; its place there
  uint32_t* count = nullptr, * start = nullptr, * cursor = nullptr;  // [inner cells]
  unsigned long long* block_sum = nullptr;  // [scan_blocks(max(n, inner cells))]
  Counts* counts = nullptr;
  uint32_t* raw_items = nullptr, * raw_cell = nullptr;  // [n_items] the items as the atomics placed them, and each one's cell
  // outputs
  rtc::SphereGeom* geom = nullptr;         // [n]
  uint32_t* cell_word = nullptr;           // [n_cells][2], wide: [n_cells][4]
  void* cell_items = nullptr;              // [n_items] u16, wide: u32
  uint32_t* large = nullptr;               // [n_large]
  rtc::SphereGeom* large_geom = nullptr;   // [n_large]
};
inline uint32_t inner_cells(const rtc::GridDesc& G) { return G.n[0] * G.n[1] * G.n[2]; }

hipError_t count(const Job& j, hipStream_t stream);
// n_items, n_large: what count() found; wide: the format the host picked with them
hipError_t tables(const Job& j, unsigned long long n_items, unsigned long long n_large, bool wide, hipStream_t stream);

}  // namespace rtgb
#endif
