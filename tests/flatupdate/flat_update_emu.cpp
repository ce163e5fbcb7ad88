// TEST INFRASTRUCTURE (tests/test_flat_update_cpu.py): pasted behind the kernels of csrc/hip/rt_flat_build.hip, which g++ compiles against
// the kernel-language emulation (tests/flatupdate/emu).  A C interface over one update of a list of flat primitives as
// rt_hip_scene_update_flats drives it — prepare(), refit(), the status block — and over the host's own rt_quad_prepare.
#include <cstdio>
using namespace rtc;

// The device path.  live_nodes / order / n_always: the structure as built for the OLD geometry (null / 0 nodes: a scene without one).
// out_rec: n x 128 B, out_nodes: n_nodes x 64 B (both pre-filled by the caller: what the kernels do not write stays), status: 4 words,
// shape: {heights, launches of flat_refit_level, bounded leaves, always-visited leaves}.
extern "C" int fu_update(const double* quv, const double* lim, uint32_t n, const void* live_nodes, uint32_t n_nodes, const uint32_t* order, uint32_t n_always,
                         void* out_rec, void* out_nodes, uint32_t* status, uint32_t* shape) {
  rtfb::Job j;
  rtfb::Status st{};
  FlatTopology tp;
  std::vector<double> box;
  const FlatNode* ln = static_cast<const FlatNode*>(live_nodes);
  j.n = n; j.quv = quv; j.lim = lim; j.rec = static_cast<RtQuadRec*>(out_rec); j.status = &st;
  if (n_nodes) {
    flat_topology(std::vector<FlatNode>(ln, ln + n_nodes), std::vector<uint32_t>(order, order + n), n_always, tp);
    box.assign(6 * (size_t)n, NAN);
    j.boxed = tp.boxed.data(); j.box = box.data();
    j.n_nodes = n_nodes; j.n_run = tp.n_run; j.n_leaves = (uint32_t)tp.leaves.size();
    j.live_nodes = ln; j.order = order; j.leaves = tp.leaves.data();
    j.level_nodes = tp.level_nodes.data(); j.level_start = tp.level_start.data(); j.n_levels = (uint32_t)tp.level_start.size() - 1u;
    j.nodes = static_cast<FlatNode*>(out_nodes);
  }
  if (rtfb::prepare(j, nullptr) != hipSuccess) return 1;
  if (n_nodes && rtfb::refit(j, nullptr) != hipSuccess) return 1;
  status[0] = st.bad_finite; status[1] = st.bad_degenerate; status[2] = st.mismatch; status[3] = st.pad;
  if (shape) {
    shape[0] = j.n_levels; shape[1] = 0; shape[2] = j.n_leaves; shape[3] = j.n_run;
    for (uint32_t h = 0; h < j.n_levels; ++h) shape[1] += tp.level_start[h + 1] > tp.level_start[h] ? 1u : 0u;
  }
  return 0;
}

// The host: rt_quad_prepare of every entry -> out_rec (untouched where refused), bad[k] = its status
extern "C" void fu_host_records(const double* quv, uint32_t n, void* out_rec, int32_t* bad) {
  RtQuadRec* rec = static_cast<RtQuadRec*>(out_rec);
  for (uint32_t k = 0; k < n; ++k) {
    RtQuadRec r;
    bad[k] = rt_quad_prepare(quv + 9 * (size_t)k, quv + 9 * (size_t)k + 3, quv + 9 * (size_t)k + 6, &r);
    if (!bad[k]) rec[k] = r;
  }
}
