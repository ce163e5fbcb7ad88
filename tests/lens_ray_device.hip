// lens_ray_device.hip — TEST PROGRAM (tests/test_lens.py), not part of the product.
// The camera rays of one pixel as the megakernel and rt_aov start them (rt_core.h lane_begin_sample), through the thin lens
// (LENS = true) and through the pinhole (LENS = false), for samples 0 .. n-1.
//     lens_ray_device IN OUT     IN: 20 f64 {origin[3], lower_left[3], horizontal[3], vertical[3], lens_u[3], lens_v[3], lens_r,
//                                            seed}, then 4 u32 {width, height, px, py}, then u32 n
//                                OUT: n x 12 f64 {lens origin[3], lens direction[3], pinhole origin[3], pinhole direction[3]}
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rust-raytracer_amd/csrc/hip/rt_core.h"

using namespace rtc;

__global__ void camera_rays(const DevScene sc, uint32_t px, uint32_t py, uint32_t n, double* out) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  Lane<false> L;
  L.ra.pixel = py * sc.width + px; L.ra.k0 = sc.seed_lo; L.ra.k1 = sc.seed_hi;
  L.s = s;
  double* o = out + 12 * (size_t)s;
  lane_begin_sample<true>(sc, L, px, py);
  o[0] = L.o.x; o[1] = L.o.y; o[2] = L.o.z; o[3] = L.d.x; o[4] = L.d.y; o[5] = L.d.z;
  lane_begin_sample<false>(sc, L, px, py);
  o[6] = L.o.x; o[7] = L.o.y; o[8] = L.o.z; o[9] = L.d.x; o[10] = L.d.y; o[11] = L.d.z;
}

#define CHK(x)                                                                                 \
  do {                                                                                         \
    hipError_t e = (x);                                                                        \
    if (e != hipSuccess) {                                                                     \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__);  \
      return 1;                                                                                \
    }                                                                                          \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: lens_ray_device IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  double cam[20];
  uint32_t px4[4], n = 0;
  const bool ok = fread(cam, 8, 20, f) == 20 && fread(px4, 4, 4, f) == 4 && fread(&n, 4, 1, f) == 1;
  fclose(f);
  if (!ok || n == 0 || n > (1u << 20) || px4[2] >= px4[0] || px4[3] >= px4[1]) { fprintf(stderr, "bad input\n"); return 2; }
  DevScene sc;
  std::memset(&sc, 0, sizeof sc);
  sc.width = px4[0]; sc.height = px4[1];
  for (int i = 0; i < 3; ++i) {
    sc.cam_origin[i] = cam[i]; sc.cam_ll[i] = cam[3 + i]; sc.cam_h[i] = cam[6 + i]; sc.cam_v[i] = cam[9 + i];
    sc.lens_u[i] = cam[12 + i]; sc.lens_v[i] = cam[15 + i];
  }
  sc.lens_r = cam[18];
  uint64_t seed;
  std::memcpy(&seed, &cam[19], 8);
  sc.seed_lo = (uint32_t)seed; sc.seed_hi = (uint32_t)(seed >> 32);
  sc.wm1 = (double)sc.width - 1.0; sc.hm1 = (double)sc.height - 1.0; sc.height_d = (double)sc.height;
  sc.cam_fast = 0;  // (the plain divisions of raytracer.rs:199-200)
  std::vector<double> out(12 * (size_t)n);
  double* d_out;
  CHK(hipMalloc(&d_out, out.size() * 8));
  hipLaunchKernelGGL(camera_rays, dim3((n + 255u) / 256u), dim3(256), 0, 0, sc, px4[2], px4[3], n, d_out);
  CHK(hipGetLastError());
  CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
  CHK(hipFree(d_out));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  fclose(f);
  return 0;
}
