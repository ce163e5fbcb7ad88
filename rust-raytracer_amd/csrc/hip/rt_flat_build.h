// rt_flat_build.h — the per-entry expressions of the structure over the flat primitives, shared by the host builder
// (rt_tables.h build_flat_bvh: what rt_hip_scene_create_flats_bvh runs) and the device code that moves the flat primitives of a resident
// scene (rt_flat_build.hip: what rt_hip_scene_update_flats runs), the static topology the refit needs, the split of the
// builder as RT_HD functions (what the device build of the order table shares with it, §26), and the device code's entry points.  Both
// sides compile these f64 expressions without contraction (-ffp-contract=off); every operation in them is correctly rounded or exact
// (+ - * / sqrt fabs compare), so they give the same bits on both.
#pragma once
#include <vector>

#include "rt_core.h"

namespace rtc {

// The padded box of entry k, or false when the entry is outside the preconditions under which the pad is derived (§22): a corner
// coordinate beyond 2^40 in magnitude, edges shorter than 2^-40, K = (|u| + |v|)^2 / |cross(u, v)| above 2^20 (extreme skew, a needle),
// anything not finite.  The box is that of the corners Q, Q + u, Q + v (and Q + u + v for a parallelogram), grown on every axis by
//     pad = 2^-20 (|u|_1 + |v|_1) + 2^-30 max |corner coordinate|:
// orders of magnitude above the rounding terms it has to cover, and never zero — an axis-aligned wall has a box of thickness 2 pad.
// (flat_min / flat_max are std::min / std::max as comparisons: the second operand only where it is strictly smaller / larger.)
constexpr double FLAT_COORD_MAX = 0x1p40, FLAT_EDGE_MIN = 0x1p-40, FLAT_SKEW_MAX = 0x1p20;
RT_HD double flat_min(double a, double b) { return b < a ? b : a; }
RT_HD double flat_max(double a, double b) { return a < b ? b : a; }
RT_HD bool flat_entry_box(const RtQuadRec& r, double lim, double lo[3], double hi[3]) {
  double l1 = 0.0, big = 0.0, edge = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double c[4] = {r.q[k], r.q[k] + r.u[k], r.q[k] + r.v[k], (r.q[k] + r.u[k]) + r.v[k]};
    const int nc = lim < 2.0 ? 3 : 4;
    lo[k] = hi[k] = c[0];
    for (int j = 0; j < nc; ++j) {
      if (!(fabs(c[j]) <= FLAT_COORD_MAX)) return false;
      lo[k] = flat_min(lo[k], c[j]); hi[k] = flat_max(hi[k], c[j]);
      big = flat_max(big, fabs(c[j]));
    }
    l1 += fabs(r.u[k]) + fabs(r.v[k]);
    edge = flat_max(edge, flat_max(fabs(r.u[k]), fabs(r.v[k])));
  }
  if (!(edge >= FLAT_EDGE_MIN)) return false;
  double n[3];
  rt_quad_cross(r.u, r.v, n);
  const double len_n = sqrt(rt_quad_dot(n, n)), len_uv = sqrt(rt_quad_dot(r.u, r.u)) + sqrt(rt_quad_dot(r.v, r.v));
  if (!(len_n > 0.0 && len_uv * len_uv <= FLAT_SKEW_MAX * len_n)) return false;
  const double pad = 0x1p-20 * l1 + 0x1p-30 * big;
  for (int k = 0; k < 3; ++k) {
    lo[k] -= pad; hi[k] += pad;
    if (!(rt_quad_finite(lo[k]) && rt_quad_finite(hi[k]))) return false;
  }
  return pad > 0.0;
}

// The box of an entry that moves within the frame (rec: its record of rt_flat_motion.h, null: it does not move): the union
// of flat_entry_box of its record at q and at q (+) m, one addition per component; false when either is outside the preconditions.  An
// entry at shutter time tau is the record at q + fl(m tau): between the two ends up to one rounding of a coordinate, which the pad of
// either end covers many orders over.  A still entry's box is flat_entry_box's in every bit.
RT_HD bool flat_entry_box_swept(const RtQuadRec& r, double lim, const double* rec, double lo[3], double hi[3]) {
  if (!flat_entry_box(r, lim, lo, hi)) return false;
  if (!rec || !rt_flat_motion_present(rec)) return true;
  RtQuadRec end;
  rt_flat_motion_end(r, rec, &end);
  double lo1[3], hi1[3];
  if (!flat_entry_box(end, lim, lo1, hi1)) return false;
  for (int k = 0; k < 3; ++k) { lo[k] = flat_min(lo[k], lo1[k]); hi[k] = flat_max(hi[k], hi1[k]); }
  return true;
}

// What a refit needs of a built structure and what follows from entry counts alone (build_flat_bvh splits at the median BY COUNT): which
// entries have a box (1) and which sit in the always-visited run (0); the bounded leaves; the inner nodes grouped by height (a leaf has
// height 0, an inner node one more than the taller of its children, node i + 1 and node nodes[i + 1].skip), the nodes of height h being
// level_nodes[level_start[h - 1] .. level_start[h]).  Derived once per build, on the host: the node order is depth first, so a child's
// index is above its parent's and one backward pass finds every height.
struct FlatTopology {
  std::vector<uint32_t> boxed;        // [n_quads]
  std::vector<uint32_t> leaves;       // the bounded leaves' node indices
  std::vector<uint32_t> level_nodes;  // the inner nodes, by height
  std::vector<uint32_t> level_start;  // [heights + 1], level_start[0] = 0
  uint32_t n_run = 0;                 // always-visited leaves: the first n_run nodes
};
inline void flat_topology(const std::vector<FlatNode>& nodes, const std::vector<uint32_t>& order, uint32_t n_always, FlatTopology& tp) {
  const uint32_t nn = (uint32_t)nodes.size();
  tp.boxed.assign(order.size(), 1u);
  for (uint32_t k = 0; k < n_always; ++k) tp.boxed[order[k]] = 0u;
  tp.n_run = (n_always + 3u) / 4u;
  tp.leaves.clear(); tp.level_nodes.clear(); tp.level_start.assign(1, 0u);
  std::vector<uint32_t> height(nn, 0u);
  uint32_t top = 0;
  for (uint32_t i = nn; i-- > tp.n_run;) {
    if (nodes[i].count) continue;
    const uint32_t l = i + 1u, r = nodes[l].skip;
    height[i] = 1u + (height[l] > height[r] ? height[l] : height[r]);
    top = height[i] > top ? height[i] : top;
  }
  std::vector<uint32_t> at(top + 1u, 0u);
  for (uint32_t i = tp.n_run; i < nn; ++i) {
    if (nodes[i].count) tp.leaves.push_back(i); else at[height[i]]++;
  }
  for (uint32_t h = 1; h <= top; ++h) tp.level_start.push_back(tp.level_start.back() + at[h]);
  tp.level_nodes.resize(tp.level_start.back());
  std::vector<uint32_t> cursor(tp.level_start.begin(), tp.level_start.end());
  for (uint32_t i = tp.n_run; i < nn; ++i)
    if (!nodes[i].count) tp.level_nodes[cursor[height[i] - 1u]++] = i;
}

// ------------------------------------------------------------------ the order table, built anew
// build_flat_bvh's split, restated so that the host builder and the device build (rt_flat_build.hip build()) run the same expressions.
// The boxed entries, m of them, start in index order at the positions 0 .. m-1; a range [a, b) of more than FLAT_LEAF_MAX positions is
// split at a + (b - a) / 2 into the (b - a) / 2 smallest entries under (centre along the axis, entry index) and the others.  Only the two
// halves AS SETS matter: the next split orders each half again and a leaf ends up in index order.
constexpr uint32_t FLAT_LEAF_MAX = 4;
RT_HD double flat_centre(double lo, double hi) { return 0.5 * lo + 0.5 * hi; }   // two products, one sum, no contraction
// the longest axis of the extent [clo, chi] of a range's centres: axis 0 unless a later one is STRICTLY longer
RT_HD int flat_split_axis(const double clo[3], const double chi[3]) {
  int axis = 0;
  for (int k = 1; k < 3; ++k) if (chi[k] - clo[k] > chi[axis] - clo[axis]) axis = k;
  return axis;
}
// the strict total order of a split: centres compared as doubles (-0.0 == 0.0: the index decides), ties by entry index
RT_HD bool flat_split_less(double cx, uint32_t x, double cy, uint32_t y) { return cx < cy || (cx == cy && x < y); }

// The range that position p (< m) lies in after `depth` splits, by count alone: [a, b) and r, its number among the ranges of that depth
// (the path from the root, left = 0).  The descent stops at a leaf.  Every range of a depth has floor or ceil of m / 2^depth positions,
// so while one of them is above FLAT_LEAF_MAX the depth before had none below 2 * FLAT_LEAF_MAX: all 2^depth ranges exist and r < 2^depth.
struct FlatRange { uint32_t a, b, r; };
RT_HD FlatRange flat_range_at(uint32_t p, uint32_t m, uint32_t depth) {
  FlatRange g = {0u, m, 0u};
  for (uint32_t d = 0; d < depth && g.b - g.a > FLAT_LEAF_MAX; ++d) {
    const uint32_t mid = g.a + (g.b - g.a) / 2u;
    if (p < mid) { g.b = mid; g.r = 2u * g.r; } else { g.a = mid; g.r = 2u * g.r + 1u; }
  }
  return g;
}
// the depths that have a range to split: the largest range of a depth is ceil(the depth before's / 2).  At most 30 for any 32-bit m.
RT_HD uint32_t flat_build_depths(uint32_t m) {
  uint32_t d = 0;
  for (uint32_t s = m; s > FLAT_LEAF_MAX; s = s / 2u + (s & 1u)) ++d;
  return d;
}
constexpr uint32_t FLAT_DEPTH_ALL = 32;   // flat_range_at(p, m, FLAT_DEPTH_ALL): the leaf of position p

// What one entry carries through the sort of one depth: the range it is in, its centre along that range's axis (0.0 in a range that is
// a leaf already: it keeps its place, in index order), itself.  flat_item_less is the comparator (range, key, index).
struct alignas(16) FlatBuildItem { double key; uint32_t seg, idx; };
static_assert(sizeof(FlatBuildItem) == 16, "an item of the device build is 16 bytes");
RT_HD bool flat_item_less(const FlatBuildItem& x, const FlatBuildItem& y) {
  return x.seg < y.seg || (x.seg == y.seg && flat_split_less(x.key, x.idx, y.key, y.idx));
}
// A double as a 64-bit word whose unsigned order is the doubles' order (-0.0 below +0.0: an extent's zero may come out with either
// sign, which neither chi - clo nor the comparison above can see), and back: the device forms a range's min and max with integer atomics.
RT_HD unsigned long long flat_ordered_bits(double x) {
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
RT_HD double flat_from_ordered_bits(unsigned long long b) {
  b = (b >> 63) ? (b & 0x7FFFFFFFFFFFFFFFull) : ~b;
  double x;
  __builtin_memcpy(&x, &b, 8);
  return x;
}
// a leaf's entries into index order (count <= FLAT_LEAF_MAX)
RT_HD void flat_leaf_sort(uint32_t* v, uint32_t count) {
  for (uint32_t i = 1; i < count; ++i)
    for (uint32_t k = i; k > 0 && v[k] < v[k - 1]; --k) { const uint32_t t = v[k]; v[k] = v[k - 1]; v[k - 1] = t; }
}

}  // namespace rtc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// The device code: per entry, its record (rt_quad.h rt_quad_prepare) and its padded box; per node, the union of what lies below it.  Two
// steps before ONE small readback (Status): prepare() and, for a scene with the structure, refit().  Every pointer is device memory; all
// work is enqueued on `stream`; a function returns the first HIP launch error.  Nothing here writes a table a frame reads: the records and
// the nodes go into spare buffers the caller swaps in after the readback said that all is well.
namespace rtfb {

constexpr uint32_t NONE = 0xFFFFFFFFu;
struct Status {              // what prepare() leaves in Job::status
  uint32_t bad_finite;       // the lowest entry with a non-finite component, or NONE
  uint32_t bad_degenerate;   // the lowest degenerate entry, or NONE
  uint32_t mismatch;         // entries whose boxed / refused flag differs from the resident one: the structure must be built anew
  uint32_t pad;              // entries that move within the frame (Job::move makes their records), or 0
};

struct Job {
  uint32_t n = 0;                           // entries
  // inputs
  const double* quv = nullptr;              // [n][9] the new q, u, v
  const double* lim = nullptr;              // [n] or null: a scene of parallelograms
  const uint32_t* boxed = nullptr;          // [n] the resident flags (FlatTopology::boxed); null: a scene without the structure
  uint32_t quv_stride = 9;                  // doubles from one entry's q to the next's: 9, or 16 for the records of a resident scene
  const double* move = nullptr;             // the displacement m of every entry over the shutter (§27), move_stride doubles apart (3: a
  uint32_t move_stride = 3;                 //   caller's; 4: a resident motion table, whose Dm is made anew); null: nothing moves
  double* motion = nullptr;                 // [n][4] the spare motion table (rt_flat_motion.h); written when move is not null
  // outputs of prepare()
  RtQuadRec* rec = nullptr;                 // [n] the spare records
  double* box = nullptr;                    // [n][6] lo, hi of every boxed entry (scratch); null without the structure
  Status* status = nullptr;
  // refit(): the live tables give the topology, the spare node table takes every node
  uint32_t n_nodes = 0, n_run = 0, n_leaves = 0;
  const rtc::FlatNode* live_nodes = nullptr;
  const uint32_t* order = nullptr;
  const uint32_t* leaves = nullptr;         // [n_leaves]
  const uint32_t* level_nodes = nullptr;    // as FlatTopology's, resident
  const uint32_t* level_start = nullptr;    // HOST memory, [n_levels + 1]
  uint32_t n_levels = 0;
  rtc::FlatNode* nodes = nullptr;           // [n_nodes] the spare node table
};

hipError_t prepare(const Job& j, hipStream_t stream);
hipError_t refit(const Job& j, hipStream_t stream);

// The order table built anew on the device, from the boxes prepare() left: per depth with a range to split, each range's
// centre extent, each entry's key, ONE sort of all boxed entries under (range, key, index); then every leaf into index order.  The node
// skeleton does not change (it follows from the counts), so a refit() over the new order table completes the structure.  Nothing is
// sized from what a kernel computed: launches, loops and offsets follow from n and m alone.
struct BuildJob {
  uint32_t n = 0, m = 0;                    // entries; those with a box (the always-visited run holds the other n - m)
  const double* box = nullptr;              // [n][6] prepare()'s
  const uint32_t* start = nullptr;          // [m] the boxed entries in index order
  const uint32_t* live_order = nullptr;     // [n] the always-visited run is copied from it
  rtc::FlatBuildItem* item = nullptr;       // [m] scratch
  unsigned long long* extent = nullptr;     // build_extent_bytes(m) of scratch
  void* sort_tmp = nullptr;                 // build_sort_bytes(m) of scratch
  size_t sort_bytes = 0;
  uint32_t* order = nullptr;                // [n] the spare order table
};
size_t build_extent_bytes(uint32_t m);
hipError_t build_sort_bytes(uint32_t m, size_t* bytes);
hipError_t build(const BuildJob& b, hipStream_t stream);

// Shading normals (rt_hip_scene_set_flat_normals): per entry, its 72-byte record by rt_flat_normal.h rt_flat_normal_prepare.
// The status block is prepare()'s: bad_finite = the lowest entry with a refused vector, bad_degenerate = the lowest parallelogram that
// carries normals, mismatch = the entries that have normals.  The records go into a spare table, like everything here.
struct NormalJob {
  uint32_t n = 0;
  const double* in = nullptr;    // [n][9] the caller's n0, n1, n2
  const double* lim = nullptr;   // [n] or null: a scene of parallelograms
  double* out = nullptr;         // [n][9]
  Status* status = nullptr;
};
hipError_t normals(const NormalJob& j, hipStream_t stream);

// Images (rt_hip_scene_set_flat_images): per entry, its 64-byte record by rt_flat_image.h rt_flat_image_prepare.  The status
// block is prepare()'s with another meaning: bad_degenerate = the lowest refused entry or NONE, bad_finite = its RT_FLAT_IMAGE_BAD_* code (a
// one-thread kernel behind the first looks the reason up again: one readback names entry and reason); mismatch = the entries that have an
// image.  The records go into a spare table, like everything here.
struct ImageJob {
  uint32_t n = 0, n_textures = 0;
  const RtFlatImage* in = nullptr;        // [n] the caller's
  const RtFlatImageTex* tex = nullptr;    // [n_textures] the scene's textures (null without any)
  const uint32_t* kind = nullptr;         // [n] the entries' own materials as created
  RtFlatImageRec* out = nullptr;          // [n]
  Status* status = nullptr;
};
hipError_t images(const ImageJob& j, hipStream_t stream);

}  // namespace rtfb
#endif
