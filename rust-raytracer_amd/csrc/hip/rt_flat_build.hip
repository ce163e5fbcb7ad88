// rt_flat_build.hip — the flat primitives of a resident scene moved on the device (rt_hip_scene_update_flats).
// flat_prepare makes each entry's record with the host's rt_quad_prepare and its padded box with the host's flat_entry_box (rt_flat_build.h),
// so the records come out byte for byte as creation makes them.  The structure is REFIT, not rebuilt: its order table and every node's skip,
// first and count stay, and a node's box becomes the union of what lies below it — leaves first, then the inner nodes height by height,
// ONE LAUNCH PER HEIGHT.  The kernel boundary is the only ordering between a child's store and its parent's load: no counter, flag or spin
// hands a box from one workgroup to another inside a launch (the L2s of the XCDs are not coherent with each other and a CU's L1 is not
// refreshed by another CU's stores; a stale box would be a silently wrong frame).  min and max are exact, so the union does not depend on
// the order it is formed in and equals the host builder's.  Plain global atomics and vector stores only.
// Behind the refit: the order table built anew on the device, for a rebuild the caller asks for.
#include <hip/hip_runtime.h>

#include "rt_flat_build.h"

namespace rtfb {
namespace {

constexpr uint32_t BLOCK = 256;

// 16-byte stores of a 128-byte record and of a 64-byte node (both 16-byte aligned: hipMalloc's alignment, sizes that are multiples of 16)
__device__ __forceinline__ void store_rec(RtQuadRec* dst, const RtQuadRec& r) {
  const double* s = reinterpret_cast<const double*>(&r);
  double2* d = reinterpret_cast<double2*>(dst);
  for (int k = 0; k < 8; ++k) d[k] = make_double2(s[2 * k], s[2 * k + 1]);
}
__device__ __forceinline__ void store_node(rtc::FlatNode* dst, const double lo[3], const double hi[3], const rtc::FlatNode& topo) {
  double2* d = reinterpret_cast<double2*>(dst);
  d[0] = make_double2(lo[0], lo[1]);
  d[1] = make_double2(lo[2], hi[0]);
  d[2] = make_double2(hi[1], hi[2]);
  reinterpret_cast<uint4*>(dst)[3] = make_uint4(topo.skip, topo.first, topo.count, topo.pad);
}

// per entry: its record into the spare records; with the structure, its padded box and whether its flag is still the resident one
__global__ void __launch_bounds__(BLOCK) flat_prepare(Job j) {
  __shared__ uint32_t changed, moved;   // of this workgroup: one global atomic per workgroup, not per lane
  if (threadIdx.x == 0) { changed = 0u; moved = 0u; }
  __syncthreads();
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < j.n) {
    const double* p = j.quv + j.quv_stride * (size_t)i;
    const double q[3] = {p[0], p[1], p[2]}, u[3] = {p[3], p[4], p[5]}, v[3] = {p[6], p[7], p[8]};
    RtQuadRec r;
    const int bad = rt_quad_prepare(q, u, v, &r);
    double mrec[4];
    int kind = RT_FLAT_MOTION_STILL;
    if (!bad && j.move) {  // (§27: the entry's motion record beside its record; a refused displacement counts as a non-finite entry)
      const double* mp = j.move + j.move_stride * (size_t)i;
      const double m[3] = {mp[0], mp[1], mp[2]};
      kind = rt_flat_motion_prepare(r, m, mrec);
    }
    if (bad == 1 || kind == RT_FLAT_MOTION_BAD) atomicMin(&j.status->bad_finite, i);
    else if (bad) atomicMin(&j.status->bad_degenerate, i);
    else {
      store_rec(j.rec + i, r);
      if (j.move) {
        double2* mo = reinterpret_cast<double2*>(j.motion + 4 * (size_t)i);
        mo[0] = make_double2(mrec[0], mrec[1]);
        mo[1] = make_double2(mrec[2], mrec[3]);
        if (kind == RT_FLAT_MOTION_MOVING) atomicAdd(&moved, 1u);
      }
      if (j.box) {
        double lo[3], hi[3];
        const bool ok = rtc::flat_entry_box_swept(r, j.lim ? j.lim[i] : 2.0, j.move ? mrec : nullptr, lo, hi);
        double2* b = reinterpret_cast<double2*>(j.box + 6 * (size_t)i);
        b[0] = make_double2(lo[0], lo[1]);
        b[1] = make_double2(lo[2], hi[0]);
        b[2] = make_double2(hi[1], hi[2]);
        if ((ok ? 1u : 0u) != j.boxed[i]) atomicAdd(&changed, 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && changed) atomicAdd(&j.status->mismatch, changed);
  if (threadIdx.x == 0 && moved) atomicAdd(&j.status->pad, moved);
}

// per bounded leaf: the union of the boxes of its up to 4 entries
__global__ void __launch_bounds__(BLOCK) flat_refit_leaves(Job j) {
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= j.n_leaves) return;
  const uint32_t i = j.leaves[k];
  if (i >= j.n_nodes) return;
  const rtc::FlatNode nd = j.live_nodes[i];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t e = 0; e < nd.count && e < 4u; ++e) {
    if (nd.first + e >= j.n) break;
    const uint32_t q = j.order[nd.first + e];
    if (q >= j.n) continue;
    const double* b = j.box + 6 * (size_t)q;
    for (int a = 0; a < 3; ++a) { lo[a] = rtc::flat_min(lo[a], b[a]); hi[a] = rtc::flat_max(hi[a], b[3 + a]); }
  }
  store_node(j.nodes + i, lo, hi, nd);
}

// per inner node of one height: the union of its two children, node i + 1 and node nodes[i + 1].skip, which earlier launches wrote
__global__ void __launch_bounds__(BLOCK) flat_refit_level(Job j, uint32_t begin, uint32_t end) {
  const uint32_t k = begin + blockIdx.x * BLOCK + threadIdx.x;
  if (k >= end) return;
  const uint32_t i = j.level_nodes[k];
  if (i + 1u >= j.n_nodes) return;
  const uint32_t l = i + 1u, r = j.live_nodes[l].skip;
  if (r >= j.n_nodes) return;
  const rtc::FlatNode a = j.nodes[l], b = j.nodes[r];
  double lo[3], hi[3];
  for (int c = 0; c < 3; ++c) { lo[c] = rtc::flat_min(a.lo[c], b.lo[c]); hi[c] = rtc::flat_max(a.hi[c], b.hi[c]); }
  store_node(j.nodes + i, lo, hi, j.live_nodes[i]);
}

// per entry: its record of shading normals into the spare table (rt_flat_normal.h: the host's bits); only a triangle may carry any
__global__ void __launch_bounds__(BLOCK) flat_normals_prepare(NormalJob j) {
  __shared__ uint32_t smooth;   // of this workgroup: one global atomic per workgroup
  if (threadIdx.x == 0) smooth = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < j.n) {
    const double* p = j.in + 9 * (size_t)i;
    double in[9], out[9];
    for (int k = 0; k < 9; ++k) in[k] = p[k];
    const int kind = rt_flat_normal_prepare(in, out);
    const bool triangle = j.lim && j.lim[i] == 1.0;
    if (kind == RT_FLAT_NORMAL_BAD) atomicMin(&j.status->bad_finite, i);
    else if (kind == RT_FLAT_NORMAL_SMOOTH && !triangle) atomicMin(&j.status->bad_degenerate, i);
    else {
      double* o = j.out + 9 * (size_t)i;
      for (int k = 0; k < 9; ++k) o[k] = out[k];
      if (kind == RT_FLAT_NORMAL_SMOOTH) atomicAdd(&smooth, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && smooth) atomicAdd(&j.status->mismatch, smooth);
}

// per entry: its image record into the spare table (rt_flat_image.h: the host's bits); the lowest refused entry into bad_degenerate
__global__ void __launch_bounds__(BLOCK) flat_images_prepare(ImageJob j) {
  __shared__ uint32_t present;   // of this workgroup: one global atomic per workgroup
  if (threadIdx.x == 0) present = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < j.n) {
    const RtFlatImage in = j.in[i];
    RtFlatImageRec out;
    const int kind = rt_flat_image_prepare(in, j.tex, j.n_textures, j.kind[i], &out);
    if (kind > RT_FLAT_IMAGE_PRESENT) atomicMin(&j.status->bad_degenerate, i);
    else {
      uint4* o = reinterpret_cast<uint4*>(j.out + i);
      double2* od = reinterpret_cast<double2*>(j.out + i);
      o[0] = make_uint4(out.texel_off, out.W, out.H, out.wrap);
      for (int k = 0; k < 3; ++k) od[1 + k] = make_double2(out.uv[2 * k], out.uv[2 * k + 1]);
      if (kind == RT_FLAT_IMAGE_PRESENT) atomicAdd(&present, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && present) atomicAdd(&j.status->mismatch, present);
}

// one thread, behind flat_images_prepare on the same stream: why the lowest refused entry was refused, into bad_finite
__global__ void flat_images_why(ImageJob j) {
  const uint32_t k = j.status->bad_degenerate;
  if (threadIdx.x != 0 || blockIdx.x != 0 || k >= j.n) return;
  RtFlatImageRec out;
  j.status->bad_finite = (uint32_t)rt_flat_image_prepare(j.in[k], j.tex, j.n_textures, j.kind[k], &out);
}

uint32_t blocks_for(uint32_t n) { return (n + BLOCK - 1) / BLOCK; }

}  // namespace

hipError_t normals(const NormalJob& j, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(j.status, 0xFF, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;   // NONE, NONE
  if ((e = hipMemsetAsync(&j.status->mismatch, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (j.n) hipLaunchKernelGGL(flat_normals_prepare, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j);
  return hipGetLastError();
}

hipError_t images(const ImageJob& j, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(j.status, 0xFF, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;   // no refused entry
  if ((e = hipMemsetAsync(&j.status->mismatch, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (j.n) {
    hipLaunchKernelGGL(flat_images_prepare, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j);
    hipLaunchKernelGGL(flat_images_why, dim3(1), dim3(1), 0, stream, j);
  }
  return hipGetLastError();
}

hipError_t prepare(const Job& j, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(j.status, 0xFF, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;   // NONE, NONE
  if ((e = hipMemsetAsync(&j.status->mismatch, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (j.n) hipLaunchKernelGGL(flat_prepare, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j);
  return hipGetLastError();
}

hipError_t refit(const Job& j, hipStream_t stream) {
  hipError_t e;
  // the always-visited leaves keep their infinite boxes: the first n_run nodes, copied as they are
  if (j.n_run && (e = hipMemcpyAsync(j.nodes, j.live_nodes, (size_t)j.n_run * sizeof(rtc::FlatNode), hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
  if (j.n_leaves) hipLaunchKernelGGL(flat_refit_leaves, dim3(blocks_for(j.n_leaves)), dim3(BLOCK), 0, stream, j);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (uint32_t h = 0; h < j.n_levels; ++h) {
    const uint32_t begin = j.level_start[h], end = j.level_start[h + 1];
    if (end > begin) hipLaunchKernelGGL(flat_refit_level, dim3(blocks_for(end - begin)), dim3(BLOCK), 0, stream, j, begin, end);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rtfb

// ------------------------------------------------------------------ the order table built anew
// build_flat_bvh's splits, depth by depth, all ranges of a depth at once.  A position's range follows from the counts (rt_flat_build.h
// flat_range_at): no table of ranges, nothing sized from what a kernel wrote.  Per depth three steps, each a launch of its own — the
// kernel boundary is again the only hand-over between workgroups: flat_build_extent forms every range's centre extent with 64-bit
// integer atomics on order-preserving bit patterns (min and max are exact: the arrival order cannot show); flat_build_keys gives every
// entry its range and its centre along the range's axis; a merge sort under flat_item_less puts each range's smaller half in front.
// (The wave intrinsics and the device-wide sort are the compiler's for the GPU only: the kernel-language emulation the CPU tests compile
// this file against stops here, and tests/flatbuild drives the same RT_HD expressions with plain loops.)
#ifdef __HIPCC__
#include <rocprim/device/device_merge_sort.hpp>

namespace rtfb {
namespace {

// the centre of entry e along axis a; an entry prepare() refused has no box (the update is dropped after the readback): any finite key
__device__ __forceinline__ double build_centre(const BuildJob& b, uint32_t e, int a) {
  const double c = rtc::flat_centre(b.box[6 * (size_t)e + a], b.box[6 * (size_t)e + 3 + a]);
  return fabs(c) <= 0x1p1000 ? c : 0.0;
}
__device__ __forceinline__ unsigned long long* build_extent_of(const BuildJob& b, uint32_t depth, uint32_t r) {
  return b.extent + 6 * ((((size_t)1 << depth) - 1u) + r);   // depth d's 2^d ranges lie behind those of the depths above
}

__global__ void __launch_bounds__(BLOCK) flat_build_start(BuildJob b) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= b.m) return;
  const uint32_t e = b.start[p];
  rtc::FlatBuildItem it;
  it.key = 0.0; it.seg = 0u; it.idx = e < b.n ? e : 0u;
  b.item[p] = it;
}

// per position: its entry's centre into the extent of its range, {min x, y, z, ~max x, y, z} as ordered bits, all by atomicMin (the
// words start as all ones).  A wave whose lanes share one range — every wave of a range of 128 positions or more but two — reduces
// across its lanes first and issues six atomics, not 384.
__global__ void __launch_bounds__(BLOCK) flat_build_extent(BuildJob b, uint32_t depth) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  rtc::FlatRange g = {0u, 0u, NONE};
  bool live = false;
  if (p < b.m) {
    g = rtc::flat_range_at(p, b.m, depth);
    live = g.b - g.a > rtc::FLAT_LEAF_MAX;
  }
  unsigned long long w[6];
  for (int k = 0; k < 6; ++k) w[k] = ~0ull;
  if (live) {
    const uint32_t e = b.item[p].idx;
    if (e < b.n)
      for (int a = 0; a < 3; ++a) {
        const unsigned long long o = rtc::flat_ordered_bits(build_centre(b, e, a));
        w[a] = o; w[3 + a] = ~o;
      }
  }
  const unsigned long long mask = __ballot(live);
  if (!mask) return;
  const int first = __ffsll((long long)mask) - 1;
  const uint32_t r0 = (uint32_t)__shfl((int)g.r, first);
  if (__all(!live || g.r == r0)) {
    for (int k = 0; k < 6; ++k)
      for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(w[k], s);
        w[k] = o < w[k] ? o : w[k];
      }
    if ((int)(threadIdx.x & 63u) == first) {
      unsigned long long* x = build_extent_of(b, depth, r0);
      for (int k = 0; k < 6; ++k) atomicMin(x + k, w[k]);
    }
  } else if (live) {
    unsigned long long* x = build_extent_of(b, depth, g.r);
    for (int k = 0; k < 6; ++k) atomicMin(x + k, w[k]);
  }
}

// per position: the item the sort of this depth orders.  In a range that is a leaf already the key is 0.0: its entries fall into index order.
__global__ void __launch_bounds__(BLOCK) flat_build_keys(BuildJob b, uint32_t depth) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= b.m) return;
  const rtc::FlatRange g = rtc::flat_range_at(p, b.m, depth);
  rtc::FlatBuildItem it = b.item[p];
  it.seg = g.r; it.key = 0.0;
  if (g.b - g.a > rtc::FLAT_LEAF_MAX && it.idx < b.n) {
    const unsigned long long* x = build_extent_of(b, depth, g.r);
    double clo[3], chi[3];
    for (int a = 0; a < 3; ++a) { clo[a] = rtc::flat_from_ordered_bits(x[a]); chi[a] = rtc::flat_from_ordered_bits(~x[3 + a]); }
    it.key = build_centre(b, it.idx, rtc::flat_split_axis(clo, chi));
  }
  b.item[p] = it;
}

// per position, the first of each leaf working: the leaf's up to 4 entries into index order, behind the always-visited run
__global__ void __launch_bounds__(BLOCK) flat_build_leaves(BuildJob b) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= b.m) return;
  const rtc::FlatRange g = rtc::flat_range_at(p, b.m, rtc::FLAT_DEPTH_ALL);
  if (p != g.a) return;
  const uint32_t count = g.b - g.a < rtc::FLAT_LEAF_MAX ? g.b - g.a : rtc::FLAT_LEAF_MAX;
  uint32_t v[rtc::FLAT_LEAF_MAX];
  for (uint32_t k = 0; k < count; ++k) v[k] = b.item[g.a + k].idx;
  rtc::flat_leaf_sort(v, count);
  uint32_t* out = b.order + (b.n - b.m) + g.a;
  for (uint32_t k = 0; k < count; ++k) out[k] = v[k];
}

struct ItemLess {
  __host__ __device__ bool operator()(const rtc::FlatBuildItem& x, const rtc::FlatBuildItem& y) const { return rtc::flat_item_less(x, y); }
};

}  // namespace

size_t build_extent_bytes(uint32_t m) { return 48u * ((((size_t)1 << rtc::flat_build_depths(m)) - 1u) + 1u); }
hipError_t build_sort_bytes(uint32_t m, size_t* bytes) {
  rtc::FlatBuildItem* none = nullptr;
  *bytes = 0;
  return m ? rocprim::merge_sort(nullptr, *bytes, none, none, (size_t)m, ItemLess()) : hipSuccess;
}

hipError_t build(const BuildJob& b, hipStream_t stream) {
  hipError_t e;
  if (b.m > b.n) return hipErrorInvalidValue;
  const uint32_t run = b.n - b.m, depths = rtc::flat_build_depths(b.m);
  // the always-visited run is in entry order and its set did not change (a changed set is Status::mismatch: the host builds)
  if (run && (e = hipMemcpyAsync(b.order, b.live_order, (size_t)run * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
  if (!b.m) return hipSuccess;
  if ((e = hipMemsetAsync(b.extent, 0xFF, build_extent_bytes(b.m), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(flat_build_start, dim3(blocks_for(b.m)), dim3(BLOCK), 0, stream, b);
  for (uint32_t d = 0; d < depths; ++d) {
    hipLaunchKernelGGL(flat_build_extent, dim3(blocks_for(b.m)), dim3(BLOCK), 0, stream, b, d);
    hipLaunchKernelGGL(flat_build_keys, dim3(blocks_for(b.m)), dim3(BLOCK), 0, stream, b, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = b.sort_bytes;
    if ((e = rocprim::merge_sort(b.sort_tmp, bytes, b.item, b.item, (size_t)b.m, ItemLess(), stream)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(flat_build_leaves, dim3(blocks_for(b.m)), dim3(BLOCK), 0, stream, b);
  return hipGetLastError();
}

}  // namespace rtfb
#endif
