// rt_grid_build.hip — the uniform grid built on the device (rt_hip_scene_update_spheres).
// The host plans the grid (rt_tables.h grid_plan: bounds, cell counts, the by-radius `large` choice); everything per (sphere, cell)
// or per cell runs here, with the expressions of rt_grid_build.h the host builder uses too, so the tables come out byte for byte as
// rt_tables.h build_grid_as makes them.  Ordering: per-cell counts are sums, so atomics give them exactly; the items of a cell are
// placed by atomics in any order and then put into ascending sphere order by a rank sort (an item's place = the number of smaller
// indices in its cell: indices are distinct), which is what the host's loop over the spheres leaves.  Plain global atomics and
// vector stores only.
#include <hip/hip_runtime.h>

#include "rt_grid_build.h"

namespace rtgb {
namespace {

constexpr uint32_t BLOCK = 256;

// per sphere: its geometry record, its cell range, and whether it ends up in `large` (the plan's flag, or a range of more cells
// than large_cell_limit)
__global__ void __launch_bounds__(BLOCK) k_ranges(Job j) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= j.n) return;
  const double c[3] = {j.centre[3 * (size_t)i], j.centre[3 * (size_t)i + 1], j.centre[3 * (size_t)i + 2]};
  const double radius = j.old_geom[i].r;
  j.geom[i] = rtc::SphereGeom{c[0], c[1], c[2], radius};
  rtc::GridRange rg;
  for (int k = 0; k < 3; ++k) { rg.a[k] = 0; rg.b[k] = -1; }
  uint32_t is_large = 1u;
  if (!j.all_large && !j.plan_large[i]) {
    const uint64_t cells = rtc::grid_cell_range(j.G, j.m, c, radius, j.motion ? j.motion + 4 * (size_t)i : nullptr, rg);
    is_large = cells > j.large_cell_limit ? 1u : 0u;
    // (the bounds hold every gridded sphere, so a range is inside the grid; one that is not lists nothing — no index leaves the tables)
    for (int k = 0; k < 3; ++k)
      if (rg.a[k] < 0 || rg.b[k] >= (int)j.G.n[k]) { rg.a[k] = 0; rg.b[k] = -1; }
  }
  j.range[i] = rg;
  j.lflag[i] = is_large;
}

// the cells sphere i is listed in, each handed to f(inner cell index): the host's loop nest and tests
template <typename F>
__device__ __forceinline__ void for_each_cell(const Job& j, uint32_t i, F f) {
  if (j.lflag[i]) return;
  const rtc::GridRange rg = j.range[i];
  const rtc::SphereGeom g = j.geom[i];
  const double c[3] = {g.cx, g.cy, g.cz};
  const bool moving = j.motion && j.motion[4 * (size_t)i + 3] != 0.0;
  for (int iz = rg.a[2]; iz <= rg.b[2]; ++iz)
    for (int iy = rg.a[1]; iy <= rg.b[1]; ++iy)
      for (int ix = rg.a[0]; ix <= rg.b[0]; ++ix) {
        if (!moving && !rtc::grid_overlaps(j.G, j.cell_w, j.m, c, g.r, ix, iy, iz)) continue;  // (a moving sphere: every cell of its swept box)
        f((uint32_t)ix + j.G.n[0] * ((uint32_t)iy + j.G.n[1] * (uint32_t)iz));
      }
}

__global__ void __launch_bounds__(BLOCK) k_count(Job j) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= j.n) return;
  for_each_cell(j, i, [&](uint32_t c) { atomicAdd(&j.count[c], 1u); });
}

__global__ void __launch_bounds__(BLOCK) k_fill(Job j, unsigned long long n_items) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= j.n) return;
  for_each_cell(j, i, [&](uint32_t c) {
    const unsigned long long p = (unsigned long long)j.start[c] + atomicAdd(&j.cursor[c], 1u);
    if (p < n_items) { j.raw_items[p] = i; j.raw_cell[p] = c; }
  });
}

// ---- exclusive scan of n u32 values in index order, in three kernels: tile sums, the scan of the tile sums (one workgroup), the tiles
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long* lds, unsigned long long* total) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < SCAN_BLOCK; d <<= 1) {
    const unsigned long long add = t >= d ? lds[t - d] : 0ull;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const unsigned long long incl = lds[t];
  if (total) *total = lds[SCAN_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_tile_sums(const uint32_t* in, uint32_t n, unsigned long long* block_sum, uint32_t* max_out) {
  __shared__ unsigned long long lds[SCAN_BLOCK];
  __shared__ uint32_t lds_max[SCAN_BLOCK];
  const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER_THREAD;
  unsigned long long s = 0;
  uint32_t mx = 0;
  for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k)
    if (base + k < n) { const uint32_t v = in[base + k]; s += v; mx = v > mx ? v : mx; }
  lds[threadIdx.x] = s; lds_max[threadIdx.x] = mx;
  __syncthreads();
  for (uint32_t d = SCAN_BLOCK / 2; d > 0; d >>= 1) {
    if (threadIdx.x < d) {
      lds[threadIdx.x] += lds[threadIdx.x + d];
      lds_max[threadIdx.x] = lds_max[threadIdx.x + d] > lds_max[threadIdx.x] ? lds_max[threadIdx.x + d] : lds_max[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    block_sum[blockIdx.x] = lds[0];
    if (max_out) atomicMax(max_out, lds_max[0]);
  }
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_sums(unsigned long long* block_sum, uint32_t n_blocks, unsigned long long* total_out) {
  __shared__ unsigned long long lds[SCAN_BLOCK];
  unsigned long long carry = 0;
  for (uint32_t b0 = 0; b0 < n_blocks; b0 += SCAN_BLOCK) {
    const uint32_t b = b0 + threadIdx.x;
    const unsigned long long v = b < n_blocks ? block_sum[b] : 0ull;
    unsigned long long total;
    const unsigned long long ex = block_exclusive(v, lds, &total);
    if (b < n_blocks) block_sum[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_tiles(const uint32_t* in, uint32_t n, const unsigned long long* block_sum, uint32_t* out) {
  __shared__ unsigned long long lds[SCAN_BLOCK];
  const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER_THREAD;
  uint32_t v[SCAN_PER_THREAD];
  unsigned long long s = 0;
  for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k) { v[k] = base + k < n ? in[base + k] : 0u; s += v[k]; }
  unsigned long long at = block_sum[blockIdx.x] + block_exclusive(s, lds, nullptr);
  for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k) {
    if (base + k < n) out[base + k] = (uint32_t)at;
    at += v[k];
  }
}

hipError_t exclusive_scan(const uint32_t* in, uint32_t* out, uint32_t n, unsigned long long* block_sum, unsigned long long* total_out,
                          uint32_t* max_out, hipStream_t stream) {
  const uint32_t blocks = (uint32_t)scan_blocks(n);
  if (blocks) hipLaunchKernelGGL(k_tile_sums, dim3(blocks), dim3(SCAN_BLOCK), 0, stream, in, n, block_sum, max_out);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_BLOCK), 0, stream, block_sum, blocks, total_out);
  if (blocks) hipLaunchKernelGGL(k_scan_tiles, dim3(blocks), dim3(SCAN_BLOCK), 0, stream, in, n, (const unsigned long long*)block_sum, out);
  return hipGetLastError();
}

// ---- the tables
// every padded cell: EXIT on the border, {first item | count << 20, no inline items yet} inside (wide: {first, count, none, 0})
__global__ void __launch_bounds__(BLOCK) k_cells(Job j, bool wide) {
  const uint32_t pc = blockIdx.x * BLOCK + threadIdx.x;
  if (pc >= j.G.n_cells) return;
  const uint32_t px = j.G.n[0] + 2, py = j.G.n[1] + 2;
  const uint32_t x = pc % px, y = (pc / px) % py, z = pc / (px * py);
  const bool inner = x >= 1 && x <= j.G.n[0] && y >= 1 && y <= j.G.n[1] && z >= 1 && z <= j.G.n[2];
  const uint32_t c = inner ? (x - 1) + j.G.n[0] * ((y - 1) + j.G.n[1] * (z - 1)) : 0u;
  if (wide) {
    uint4 w = make_uint4(rtc::CELL_EXIT, 0u, rtc::CELL_NO_ITEM32, 0u);
    if (inner) { w.x = j.start[c]; w.y = j.count[c]; }
    reinterpret_cast<uint4*>(j.cell_word)[pc] = w;
  } else {
    uint2 w = make_uint2(rtc::CELL_EXIT, rtc::CELL_EXIT);
    if (inner) w.x = j.start[c] | (j.count[c] << rtc::CELL_COUNT_SHIFT);  // (w.y: no first item, no second — k_sort writes the halves that exist)
    reinterpret_cast<uint2*>(j.cell_word)[pc] = w;
  }
}

// per item as the atomics placed it: its rank among the items of its cell is its place in the cell's list; the first two of a
// cell (wide: the first) are copied into the cell's entry as well
__global__ void __launch_bounds__(BLOCK) k_sort(Job j, unsigned long long n_items, bool wide) {
  const unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n_items) return;
  const uint32_t c = j.raw_cell[p], v = j.raw_items[p];
  const uint32_t first = j.start[c], cnt = j.count[c];
  uint32_t rank = 0;
  for (uint32_t q = 0; q < cnt; ++q) rank += j.raw_items[first + q] < v ? 1u : 0u;
  const unsigned long long at = (unsigned long long)first + rank;
  if (at >= n_items) return;
  const uint32_t px = j.G.n[0] + 2, py = j.G.n[1] + 2;
  const uint32_t ix = c % j.G.n[0], iy = (c / j.G.n[0]) % j.G.n[1], iz = c / (j.G.n[0] * j.G.n[1]);
  const size_t pc = (ix + 1) + (size_t)px * ((iy + 1) + py * (iz + 1));
  if (wide) {
    static_cast<uint32_t*>(j.cell_items)[at] = v;
    if (rank == 0) j.cell_word[4 * pc + 2] = v;
  } else {
    static_cast<uint16_t*>(j.cell_items)[at] = (uint16_t)v;
    if (rank < 2) reinterpret_cast<uint16_t*>(j.cell_word)[2 * (2 * pc + 1) + rank] = (uint16_t)v;  // (i0 | i1 << 16, little endian)
  }
}

__global__ void __launch_bounds__(BLOCK) k_large(Job j, unsigned long long n_large) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= j.n || !j.lflag[i]) return;
  const uint32_t at = j.lpos[i];
  if (at >= n_large) return;
  j.large[at] = i;
  j.large_geom[at] = j.geom[i];
}

uint32_t blocks_for(unsigned long long n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }

}  // namespace

hipError_t count(const Job& j, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(j.counts, 0, sizeof(Counts), stream)) != hipSuccess) return e;
  if (j.n) hipLaunchKernelGGL(k_ranges, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t inner = j.all_large ? 0u : inner_cells(j.G);
  if (inner) {
    if ((e = hipMemsetAsync(j.count, 0, (size_t)inner * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(j.cursor, 0, (size_t)inner * 4, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_count, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = exclusive_scan(j.count, j.start, inner, j.block_sum, &j.counts->n_items, &j.counts->max_count, stream)) != hipSuccess) return e;
  }
  return exclusive_scan(j.lflag, j.lpos, j.n, j.block_sum, &j.counts->n_large, nullptr, stream);
}

hipError_t tables(const Job& j, unsigned long long n_items, unsigned long long n_large, bool wide, hipStream_t stream) {
  hipError_t e;
  if (!j.all_large && j.G.n_cells) {
    hipLaunchKernelGGL(k_cells, dim3(blocks_for(j.G.n_cells)), dim3(BLOCK), 0, stream, j, wide);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n_items) {
      hipLaunchKernelGGL(k_fill, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j, n_items);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      hipLaunchKernelGGL(k_sort, dim3(blocks_for(n_items)), dim3(BLOCK), 0, stream, j, n_items, wide);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  if (n_large) hipLaunchKernelGGL(k_large, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j, n_large);
  return hipGetLastError();
}

}  // namespace rtgb
