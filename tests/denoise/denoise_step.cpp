// denoise_step.cpp — TEST TOOL, not part of the product.  The denoising filter's per-pixel step (rust-raytracer_amd/csrc/hip/rt_core.h
// denoise_consts / denoise_pixel / linear_to_u8) built for the CPU with -ffp-contract=off and driven over a whole frame one pixel at a
// time, the iterations ping-ponging like rt_hip_denoise's.  tests/test_denoise.py compares it with the numpy restatement.
#include <cstdint>
#include <vector>

#include "../../rust-raytracer_amd/csrc/hip/rt_core.h"

using namespace rtc;

namespace {
struct HostSrc {
  const float* col;  // 3 floats per pixel
  const float* aov;  // 8 floats per pixel
  DnColour colour(size_t i) const { DnColour c; c.r = col[3 * i]; c.g = col[3 * i + 1]; c.b = col[3 * i + 2]; return c; }
  DnGuide guide(size_t i) const {
    DnGuide g;
    for (int k = 0; k < 3; ++k) { g.a[k] = aov[8 * i + k]; g.n[k] = aov[8 * i + 4 + k]; }
    g.iz = aov[8 * i + 3]; g.cov = aov[8 * i + 7];
    return g;
  }
};
}  // namespace

extern "C" void denoise_step_frame(const float* lin, const float* aov, uint32_t width, uint32_t height, uint32_t iterations,
                                   const float sigma[4], float* out_linear, uint8_t* out_rgb8) {
  const size_t n = (size_t)width * height;
  std::vector<float> a(lin, lin + 3 * n), b(3 * n);
  for (uint32_t i = 0; i < iterations; ++i) {
    const DenoiseK k = denoise_consts(i, sigma[0], sigma[1], sigma[2], sigma[3]);
    const HostSrc src{a.data(), aov};
    for (uint32_t y = 0; y < height; ++y)
      for (uint32_t x = 0; x < width; ++x) {
        const DnColour o = denoise_pixel(src, width, height, x, y, 1u << i, k);
        const size_t p = (size_t)y * width + x;
        b[3 * p] = o.r; b[3 * p + 1] = o.g; b[3 * p + 2] = o.b;
      }
    a.swap(b);
  }
  for (size_t e = 0; e < 3 * n; ++e) { out_linear[e] = a[e]; out_rgb8[e] = linear_to_u8(a[e]); }
}

extern "C" float denoise_step_w(float x) { return denoise_w(x); }
