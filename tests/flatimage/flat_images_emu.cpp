// TEST INFRASTRUCTURE (tests/test_flat_image_cpu.py): pasted behind the kernels of csrc/hip/rt_flat_build.hip, which g++ compiles
// against the kernel-language emulation (tests/flatupdate/emu).  A C interface over rtfb::images() — the device path of
// rt_hip_scene_set_flat_images with its status block — and over the host's own rt_flat_image_prepare.
using namespace rtc;

// out: n x 64 B, pre-filled by the caller (what the kernel does not write stays); status: {the reason of the lowest refused entry, that
// entry, entries with an image, pad}
extern "C" int fie_device(const RtFlatImage* in, uint32_t n, const void* tex, uint32_t n_textures, const uint32_t* kind, void* out, uint32_t* status) {
  rtfb::ImageJob j;
  rtfb::Status st{};
  j.n = n; j.n_textures = n_textures; j.in = in; j.tex = static_cast<const RtFlatImageTex*>(tex); j.kind = kind;
  j.out = static_cast<RtFlatImageRec*>(out); j.status = &st;
  if (rtfb::images(j, nullptr) != hipSuccess) return 1;
  status[0] = st.bad_finite; status[1] = st.bad_degenerate; status[2] = st.mismatch; status[3] = st.pad;
  return 0;
}

// the host path: rt_flat_image_prepare of every entry -> out (untouched where refused), code[k]
extern "C" void fie_host(const RtFlatImage* in, uint32_t n, const void* tex, uint32_t n_textures, const uint32_t* kind, void* out, int32_t* code) {
  RtFlatImageRec* o = static_cast<RtFlatImageRec*>(out);
  for (uint32_t k = 0; k < n; ++k) {
    RtFlatImageRec rec;
    code[k] = rt_flat_image_prepare(in[k], static_cast<const RtFlatImageTex*>(tex), n_textures, kind[k], &rec);
    if (code[k] <= RT_FLAT_IMAGE_PRESENT) o[k] = rec;
  }
}
