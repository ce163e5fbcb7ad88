// flat_build_emu.cpp — TEST TOOL (tests/test_flat_device_build_cpu.py), not part of the product.  The order table as the device build of
// csrc/hip/rt_flat_build.hip makes it, on the host: the same RT_HD expressions of rt_flat_build.h — flat_centre,
// flat_range_at, flat_ordered_bits, flat_split_axis, flat_item_less, flat_leaf_sort — step by step as build() enqueues them, with a plain
// loop over the positions where a kernel has one thread per position and std::sort under flat_item_less where the device sorts.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../rust-raytracer_amd/csrc/hip/rt_flat_build.h"

using namespace rtc;

// boxes lo / hi [n x 3], ok[n] (0: a refused entry, in the always-visited run) -> order[n]; info = {boxed entries, depths};
// axes[d]: which axes (bit k) the ranges of depth d split along.  Returns 0.
extern "C" int fbd_build(const double* lo, const double* hi, const int32_t* ok, uint32_t n, uint32_t* order, uint32_t* info, uint32_t* axes) {
  std::vector<uint32_t> start;
  uint32_t run = 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (ok[k]) start.push_back(k); else order[run++] = k;
  }
  const uint32_t m = (uint32_t)start.size(), depths = flat_build_depths(m);
  info[0] = m; info[1] = depths;
  std::vector<FlatBuildItem> item(m);
  for (uint32_t p = 0; p < m; ++p) { item[p].key = 0.0; item[p].seg = 0u; item[p].idx = start[p]; }
  for (uint32_t d = 0; d < depths; ++d) {
    std::vector<unsigned long long> extent(6 * ((size_t)1 << d), ~0ull);
    for (uint32_t p = 0; p < m; ++p) {   // flat_build_extent
      const FlatRange g = flat_range_at(p, m, d);
      if (g.b - g.a <= FLAT_LEAF_MAX) continue;
      const uint32_t e = item[p].idx;
      for (int a = 0; a < 3; ++a) {
        const unsigned long long o = flat_ordered_bits(flat_centre(lo[3 * e + a], hi[3 * e + a]));
        unsigned long long* x = extent.data() + 6 * (size_t)g.r;
        x[a] = std::min(x[a], o); x[3 + a] = std::min(x[3 + a], ~o);
      }
    }
    axes[d] = 0u;
    for (uint32_t p = 0; p < m; ++p) {   // flat_build_keys
      const FlatRange g = flat_range_at(p, m, d);
      item[p].seg = g.r; item[p].key = 0.0;
      if (g.b - g.a <= FLAT_LEAF_MAX) continue;
      const unsigned long long* x = extent.data() + 6 * (size_t)g.r;
      double clo[3], chi[3];
      for (int a = 0; a < 3; ++a) { clo[a] = flat_from_ordered_bits(x[a]); chi[a] = flat_from_ordered_bits(~x[3 + a]); }
      const int axis = flat_split_axis(clo, chi);
      axes[d] |= 1u << axis;
      item[p].key = flat_centre(lo[3 * item[p].idx + axis], hi[3 * item[p].idx + axis]);
    }
    std::sort(item.begin(), item.end(), [](const FlatBuildItem& x, const FlatBuildItem& y) { return flat_item_less(x, y); });
  }
  for (uint32_t p = 0; p < m; ++p) {     // flat_build_leaves
    const FlatRange g = flat_range_at(p, m, FLAT_DEPTH_ALL);
    if (p != g.a) continue;
    uint32_t v[FLAT_LEAF_MAX];
    const uint32_t count = g.b - g.a;
    if (count > FLAT_LEAF_MAX) return 1;
    for (uint32_t k = 0; k < count; ++k) v[k] = item[g.a + k].idx;
    flat_leaf_sort(v, count);
    for (uint32_t k = 0; k < count; ++k) order[run + g.a + k] = v[k];
  }
  return 0;
}

// flat_ordered_bits of x[n] and the way back
extern "C" void fbd_ordered_bits(const double* x, uint32_t n, unsigned long long* bits, double* back) {
  for (uint32_t k = 0; k < n; ++k) { bits[k] = flat_ordered_bits(x[k]); back[k] = flat_from_ordered_bits(bits[k]); }
}
