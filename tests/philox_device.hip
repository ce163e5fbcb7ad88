// philox_device.hip — TEST PROGRAM (tests/test_philox_device.py), not part of the product.
// Runs the megakernel's Philox4x32-10 (rt_core.h) on the GPU over counters and keys read from a file, in both forms the
// device code compiles it to:
//   [0] rng(): the key made wave-uniform (readfirstlane), so each round's three-input XOR takes the key as its SGPR operand
//       — the form of every draw of the megakernel.  The caller gives every aligned group of 64 entries one key.
//   [1] philox4x32_10() with a per-lane key: all three XOR operands in VGPRs.
//     philox_device IN OUT     IN: uint32 n (a multiple of 64), then n x 4 counter words, then n x 2 key words
//                              OUT: n x 4 words of form [0], then n x 4 words of form [1]
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../rust-raytracer_amd/csrc/hip/rt_core.h"

using namespace rtc;

__global__ void philox_both(const uint32_t* ctr, const uint32_t* key, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c0 = ctr[4 * i], c1 = ctr[4 * i + 1], c2 = ctr[4 * i + 2], c3 = ctr[4 * i + 3];
  RngAddr a;
  a.pixel = c0; a.sample = c1; a.k0 = key[2 * i]; a.k1 = key[2 * i + 1];
  const U4 u = rng(a, c2, c3);
  const U4 v = philox4x32_10(c0, c1, c2, c3, a.k0, a.k1);
  uint32_t* o = out + 4 * (size_t)i;
  o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w;
  o += 4 * (size_t)n;
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
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
  if (argc != 3) { fprintf(stderr, "usage: philox_device IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n == 0 || n % 64u != 0 || n > (1u << 24)) { fprintf(stderr, "bad n\n"); fclose(f); return 2; }
  std::vector<uint32_t> ctr(4 * (size_t)n), key(2 * (size_t)n), out(8 * (size_t)n);
  const bool ok = fread(ctr.data(), 4, ctr.size(), f) == ctr.size() && fread(key.data(), 4, key.size(), f) == key.size();
  fclose(f);
  if (!ok) { fprintf(stderr, "short input\n"); return 2; }
  uint32_t *d_ctr, *d_key, *d_out;
  CHK(hipMalloc(&d_ctr, ctr.size() * 4));
  CHK(hipMalloc(&d_key, key.size() * 4));
  CHK(hipMalloc(&d_out, out.size() * 4));
  CHK(hipMemcpy(d_ctr, ctr.data(), ctr.size() * 4, hipMemcpyHostToDevice));
  CHK(hipMemcpy(d_key, key.data(), key.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(philox_both, dim3((n + 255u) / 256u), dim3(256), 0, 0, d_ctr, d_key, n, d_out);
  CHK(hipGetLastError());
  CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
  CHK(hipFree(d_ctr));
  CHK(hipFree(d_key));
  CHK(hipFree(d_out));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  fclose(f);
  return 0;
}
