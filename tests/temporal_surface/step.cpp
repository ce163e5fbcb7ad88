// step.cpp — TEST TOOL, not part of the product.  The reprojection step of temporal denoising with surface tracking
// (rust-raytracer_amd/csrc/hip/rt_core.h reproject_surface_pixel) built for the CPU with -ffp-contract=off and driven
// over a whole frame one pixel at a time.  tests/test_temporal_surface_cpu.py compares it with the numpy restatement
// (tests/temporal_surface_ref.py); the surface record itself (surface_pixel) comes from tests/lanesim/.
#include <cstdint>

#include "../../rust-raytracer_amd/csrc/hip/rt_core.h"

using namespace rtc;

namespace {
struct HostSrc {
  const float* col;       // 3 floats per pixel
  const float* aov;       // 8 floats per pixel
  const float* prev_h;    // 4 floats per pixel
  const float* prev_aov;  // 8 floats per pixel
  const SurfRec* s;       // 16 bytes per pixel
  const SurfRec* prev_s;
  static DnGuide load(const float* a, size_t i) {
    DnGuide g;
    for (int k = 0; k < 3; ++k) { g.a[k] = a[8 * i + k]; g.n[k] = a[8 * i + 4 + k]; }
    g.iz = a[8 * i + 3]; g.cov = a[8 * i + 7];
    return g;
  }
  DnColour colour(size_t i) const { DnColour c; c.r = col[3 * i]; c.g = col[3 * i + 1]; c.b = col[3 * i + 2]; return c; }
  DnGuide guide(size_t i) const { return load(aov, i); }
  DnGuide prev_guide(size_t i) const { return load(prev_aov, i); }
  RpHist prev_hist(size_t i) const { RpHist h; h.r = prev_h[4 * i]; h.g = prev_h[4 * i + 1]; h.b = prev_h[4 * i + 2]; h.n = prev_h[4 * i + 3]; return h; }
  SurfRec surf(size_t i) const { return s[i]; }
  SurfRec prev_surf(size_t i) const { return prev_s[i]; }
};
ReprojCam cam_of(const double c[12]) {
  ReprojCam r;
  for (int i = 0; i < 3; ++i) { r.o[i] = c[i]; r.ll[i] = c[3 + i]; r.h[i] = c[6 + i]; r.v[i] = c[9 + i]; }
  return r;
}
}  // namespace

static_assert(sizeof(SurfRec) == 16, "the surface record is 16 bytes");

// params = alpha_min, alpha_specular, n_max, tau_n, tau_a, tau_z; disp: null or n_disp x 3
extern "C" void surface_step_frame(const float* lin, const float* aov, const void* surf, const float* prev_hist, const float* prev_aov, const void* prev_surf,
                                   const double cam[12], const double prev_cam[12], const double* disp, uint32_t n_disp, uint32_t width, uint32_t height,
                                   const float params[6], float* out_hist) {
  const HostSrc src{lin, aov, prev_hist, prev_aov, static_cast<const SurfRec*>(surf), static_cast<const SurfRec*>(prev_surf)};
  const ReprojCam cur = cam_of(cam), prev = cam_of(prev_cam);
  const ReprojSurfK k{params[0], params[1], params[2], params[3], params[4], params[5]};
  for (uint32_t y = 0; y < height; ++y)
    for (uint32_t x = 0; x < width; ++x) {
      const RpHist o = reproject_surface_pixel(src, cur, prev, disp, n_disp, width, height, x, y, k);
      float* d = out_hist + 4 * ((size_t)y * width + x);
      d[0] = o.r; d[1] = o.g; d[2] = o.b; d[3] = o.n;
    }
}
