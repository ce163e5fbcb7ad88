// TEST INFRASTRUCTURE (tests/test_smooth_prepare_cpu.py): pasted behind the kernels of csrc/hip/rt_flat_build.hip, which g++ compiles
// against the kernel-language emulation (tests/flatupdate/emu).  A C interface over rtfb::normals() — the device path of
// rt_hip_scene_set_flat_normals with its status block — and over the host's own rt_flat_normal_prepare.
using namespace rtc;

// out: n x 72 B, pre-filled by the caller (what the kernel does not write stays); status: {lowest refused vector, lowest parallelogram
// with normals, entries with normals, pad}
extern "C" int fn_device(const double* in, const double* lim, uint32_t n, double* out, uint32_t* status) {
  rtfb::NormalJob j;
  rtfb::Status st{};
  j.n = n; j.in = in; j.lim = lim; j.out = out; j.status = &st;
  if (rtfb::normals(j, nullptr) != hipSuccess) return 1;
  status[0] = st.bad_finite; status[1] = st.bad_degenerate; status[2] = st.mismatch; status[3] = st.pad;
  return 0;
}

// the host path: rt_flat_normal_prepare of every entry -> out (untouched where refused), kind[k]
extern "C" void fn_host(const double* in, uint32_t n, double* out, int32_t* kind) {
  for (uint32_t k = 0; k < n; ++k) {
    double rec[9];
    kind[k] = rt_flat_normal_prepare(in + 9 * (size_t)k, rec);
    if (kind[k] != RT_FLAT_NORMAL_BAD)
      for (int c = 0; c < 9; ++c) out[9 * (size_t)k + c] = rec[c];
  }
}
