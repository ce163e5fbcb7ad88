// TEST INFRASTRUCTURE (tests/test_flat_motion_cpu.py): pasted behind the kernels of csrc/hip/rt_flat_build.hip, which g++ compiles against
// the kernel-language emulation (tests/flatupdate/emu), as tests/flatupdate/flat_update_emu.cpp is.  One update of a list of flat
// primitives that move within the frame as rt_hip_scene_set_flat_motion and rt_hip_scene_update_flats drive it: prepare()
// with Job::move, then refit() over the structure the host built.
#include <cstdio>
using namespace rtc;

// quv: n x quv_stride doubles (9: a caller's; 16: resident records); move: n x move_stride doubles (3: a caller's; 4: a resident motion
// table).  live_nodes / order / n_always: the structure as the host built it.  out_rec n x 128 B, out_motion n x 4, out_box n x 6,
// out_nodes n_nodes x 64 B (pre-filled by the caller), status 4 words.
extern "C" int fme_update(const double* quv, uint32_t quv_stride, const double* lim, const double* move, uint32_t move_stride, uint32_t n, const void* live_nodes,
                          uint32_t n_nodes, const uint32_t* order, uint32_t n_always, void* out_rec, double* out_motion, double* out_box, void* out_nodes,
                          uint32_t* status) {
  rtfb::Job j;
  rtfb::Status st{};
  FlatTopology tp;
  const FlatNode* ln = static_cast<const FlatNode*>(live_nodes);
  j.n = n; j.quv = quv; j.quv_stride = quv_stride; j.lim = lim; j.rec = static_cast<RtQuadRec*>(out_rec); j.status = &st;
  j.move = move; j.move_stride = move_stride; j.motion = out_motion;
  flat_topology(std::vector<FlatNode>(ln, ln + n_nodes), std::vector<uint32_t>(order, order + n), n_always, tp);
  j.boxed = tp.boxed.data(); j.box = out_box;
  j.n_nodes = n_nodes; j.n_run = tp.n_run; j.n_leaves = (uint32_t)tp.leaves.size();
  j.live_nodes = ln; j.order = order; j.leaves = tp.leaves.data();
  j.level_nodes = tp.level_nodes.data(); j.level_start = tp.level_start.data(); j.n_levels = (uint32_t)tp.level_start.size() - 1u;
  j.nodes = static_cast<FlatNode*>(out_nodes);
  if (rtfb::prepare(j, nullptr) != hipSuccess) return 1;
  if (rtfb::refit(j, nullptr) != hipSuccess) return 1;
  status[0] = st.bad_finite; status[1] = st.bad_degenerate; status[2] = st.mismatch; status[3] = st.pad;
  return 0;
}
