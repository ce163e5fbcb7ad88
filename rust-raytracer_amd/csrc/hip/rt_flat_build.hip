// rt_flat_build.hip — the flat primitives of a resident scene moved on the device (rt_hip_scene_update_flats).
// flat_prepare makes each entry's record with the host's rt_quad_prepare and its padded box with the host's flat_entry_box (rt_flat_build.h),
// so the records come out byte for byte as creation makes them.  The structure is REFIT, not rebuilt: its order table and every node's skip,
// first and count stay, and a node's box becomes the union of what lies below it — leaves first, then the inner nodes height by height,
// ONE LAUNCH PER HEIGHT.  The kernel boundary is the only ordering between a child's store and its parent's load: no counter, flag or spin
// hands a box from one workgroup to another inside a launch (the L2s of the XCDs are not coherent with each other and a CU's L1 is not
// refreshed by another CU's stores; a stale box would be a silently wrong frame).  min and max are exact, so the union does not depend on
// the order it is formed in and equals the host builder's.  Plain global atomics and vector stores only.
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
  __shared__ uint32_t changed;   // of this workgroup: one global atomic per workgroup, not per lane
  if (threadIdx.x == 0) changed = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < j.n) {
    const double* p = j.quv + 9 * (size_t)i;
    const double q[3] = {p[0], p[1], p[2]}, u[3] = {p[3], p[4], p[5]}, v[3] = {p[6], p[7], p[8]};
    RtQuadRec r;
    const int bad = rt_quad_prepare(q, u, v, &r);
    if (bad == 1) atomicMin(&j.status->bad_finite, i);
    else if (bad) atomicMin(&j.status->bad_degenerate, i);
    else {
      store_rec(j.rec + i, r);
      if (j.box) {
        double lo[3], hi[3];
        const bool ok = rtc::flat_entry_box(r, j.lim ? j.lim[i] : 2.0, lo, hi);
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

uint32_t blocks_for(uint32_t n) { return (n + BLOCK - 1) / BLOCK; }

}  // namespace

hipError_t normals(const NormalJob& j, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(j.status, 0xFF, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;   // NONE, NONE
  if ((e = hipMemsetAsync(&j.status->mismatch, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (j.n) hipLaunchKernelGGL(flat_normals_prepare, dim3(blocks_for(j.n)), dim3(BLOCK), 0, stream, j);
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
