// flat_motion_main.cpp — TEST TOOL, not part of the product.  A stand-alone program (its own main, no Python in the process) over the host
// code of flat primitives that move within the frame: the header, the swept boxes, the builder, the traversal beside the
// scan, and the loader and writer of "move".  tests/test_flat_motion_sanitizers.py builds it with ASan + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../include/rt_abi.h"
#include "flat_motion_sim.cpp"

namespace {
int fail(const char* what) { std::fprintf(stderr, "FAILED: %s\n", what); return 1; }
}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  uint64_t differ = 0, hits = 0, inside = 0;
  for (uint32_t n : {1u, 4u, 5u, 33u, 257u}) {
    std::vector<RtQuad> quads(n);
    std::vector<double> move(3 * (size_t)n, 0.0);
    for (uint32_t k = 0; k < n; ++k) {
      RtQuad& q = quads[k];
      std::memset(&q, 0, sizeof q);
      for (int c = 0; c < 3; ++c) { q.q[c] = 8.0 * U(rng); q.u[c] = 2.0 * U(rng); q.v[c] = 2.0 * U(rng); }
      q.reserved = k & 1u;
      if (k % 2 == 0) for (int c = 0; c < 3; ++c) move[3 * (size_t)k + c] = 3.0 * U(rng);
      if (k % 16 == 7) move[3 * (size_t)k] = 0x1p41;   // outside the preconditions at the far end only
    }
    const uint64_t n_rays = 4000;
    std::vector<double> rays(6 * n_rays), closest(n_rays, 1e300), t0(n_rays), t1(n_rays);
    std::vector<float> tau(n_rays);
    std::vector<int32_t> b0(n_rays), b1(n_rays);
    for (uint64_t i = 0; i < n_rays; ++i) {
      for (int c = 0; c < 3; ++c) { rays[6 * i + c] = 12.0 * U(rng); rays[6 * i + 3 + c] = U(rng); }
      tau[i] = (float)(rng() >> 40) * 0x1p-24f;
    }
    uint64_t count[5];
    if (fm_list_hit(quads.data(), n, move.data(), 3u, 0, rays.data(), tau.data(), closest.data(), nullptr, n_rays, b0.data(), t0.data(), count)) return fail("scan");
    if (fm_list_hit(quads.data(), n, move.data(), 3u, 1, rays.data(), tau.data(), closest.data(), nullptr, n_rays, b1.data(), t1.data(), count)) return fail("structure");
    for (uint64_t i = 0; i < n_rays; ++i) {
      differ += b0[i] != b1[i] || std::memcmp(&t0[i], &t1[i], 8) != 0;
      hits += b0[i] >= 0;
    }
    // every accepted hit point lies in its entry's swept box
    std::vector<int32_t> ok(n);
    std::vector<double> lo(3 * (size_t)n), hi(3 * (size_t)n);
    if (fm_boxes(quads.data(), n, move.data(), ok.data(), lo.data(), hi.data())) return fail("boxes");
    for (uint64_t i = 0; i < n_rays; ++i) {
      if (b0[i] < 3) continue;
      const uint32_t k = (uint32_t)b0[i] - 3u;
      if (!ok[k]) continue;
      bool in = true;
      for (int c = 0; c < 3; ++c) {
        const double p = rays[6 * i + c] + rays[6 * i + 3 + c] * t0[i];
        in = in && lo[3 * k + c] <= p && p <= hi[3 * k + c];
      }
      inside += in;
      if (!in) return fail("a hit point outside its swept box");
    }
  }
  if (differ) return fail("the structure and the scan differ");
  // the loader and the writer: all four forms, both point forms; load -> write -> load is bit for bit
  const char* text =
      "{\"width\":8,\"height\":8,\"samples_per_pixel\":1,\"max_depth\":4,\"sky\":null,"
      "\"camera\":{\"look_from\":{\"x\":0,\"y\":0,\"z\":5},\"look_at\":{\"x\":0,\"y\":0,\"z\":0},\"vup\":{\"x\":0,\"y\":1,\"z\":0},\"vfov\":40,\"aspect\":1},"
      "\"objects\":[{\"q\":[0,0,0],\"u\":[1,0,0],\"v\":[0,1,0],\"move\":[0.25,0,0],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"triangle\":[[0,0,1],[1,0,1],[0,1,1]],\"move\":{\"x\":0,\"y\":-0.5,\"z\":0.125},\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"box\":{\"min\":[1,1,1],\"max\":[2,2,2]},\"move\":[0,-1,0],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"mesh\":{\"vertices\":[[0,0,2],[1,0,2],[0,1,2],[1,1,2]],\"faces\":[[0,1,2],[1,3,2]]},\"move\":[0.1,0.2,0.3],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"q\":[0,0,3],\"u\":[1,0,0],\"v\":[0,1,0],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}}]}";
  RtSceneFile *a = nullptr, *b = nullptr;
  if (rt_scene_load_string(text, std::strlen(text), &a) != RT_OK) return fail(rt_host_last_error());
  uint32_t na = 0, nb = 0;
  const double* ma = rt_scene_flat_motion(a, &na);
  if (!ma || na != 11u) return fail("rt_scene_flat_motion: expected 11 entries");
  size_t need = 0;
  rt_scene_to_json(a, nullptr, 0, &need);
  std::vector<char> buf(need);
  if (rt_scene_to_json(a, buf.data(), need, nullptr) != RT_OK) return fail("rt_scene_to_json");
  if (rt_scene_load_string(buf.data(), std::strlen(buf.data()), &b) != RT_OK) return fail(rt_host_last_error());
  const double* mb = rt_scene_flat_motion(b, &nb);
  if (!mb || nb != na || std::memcmp(ma, mb, 24 * (size_t)na)) return fail("the round trip changed the motion");
  rt_scene_free(a); rt_scene_free(b);
  std::printf("flat motion: %llu hits, %llu inside their swept boxes, structure == scan, round trip of %u entries\n", (unsigned long long)hits,
              (unsigned long long)inside, na);
  return 0;
}
