// flat_light_main.cpp — TEST TOOL, not part of the product.  A stand-alone program (its own main, no Python in the process) over the host
// code of flat primitives that emit: the header's aim on the class tables of tests/test_flat_light_cpu.py (generic entries,
// a + b at 1, the words' extremes, needles, huge and tiny magnitudes), the emit validation, a small lit frame of the lane code, and the loader
// and writer of "emit".  tests/test_flat_light_cpu.py builds it with ASan + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../include/rt_abi.h"
#include "flat_light_sim.cpp"

namespace {
int fail(const char* what) { std::fprintf(stderr, "FAILED: %s\n", what); return 1; }
}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const uint64_t n = 100000;
  std::vector<double> quv(9 * n), T(3 * n), ab(2 * n);
  std::vector<int32_t> tri(n);
  std::vector<uint32_t> words(4 * n);
  uint64_t folded = 0, outside = 0;
  for (int cls = 0; cls < 5; ++cls) {
    for (uint64_t i = 0; i < n; ++i) {
      const double scale = cls == 3 ? 1e150 : (cls == 4 ? 1e-150 : 1.0);
      for (int c = 0; c < 9; ++c) quv[9 * i + c] = scale * 4.0 * U(rng);
      if (cls == 2) for (int c = 0; c < 3; ++c) quv[9 * i + 6 + c] = quv[9 * i + 3 + c] * (1.0 + 1e-9 * U(rng));   // a needle: v nearly u
      tri[i] = (int32_t)(i & 1u);
      for (int c = 0; c < 4; ++c) words[4 * i + c] = (uint32_t)rng();
      if (cls == 1) {  // a + b within ulps of 1, or a word pair at an extreme
        const uint64_t a = rng() >> 11, d = (i % 7) - 3;
        const uint64_t b = ((1ull << 53) - a + d) & ((1ull << 53) - 1);
        words[4 * i] = (uint32_t)(a << 11); words[4 * i + 1] = (uint32_t)((a << 11) >> 32);
        words[4 * i + 2] = (uint32_t)(b << 11); words[4 * i + 3] = (uint32_t)((b << 11) >> 32);
        if (i % 5 == 0) { words[4 * i] = words[4 * i + 1] = (i % 10) ? 0xFFFFFFFFu : 0u; }
      }
    }
    fl_aim(quv.data(), tri.data(), words.data(), n, T.data());
    fl_ab(words.data(), n, ab.data());
    for (uint64_t i = 0; i < n; ++i) {
      double a = ab[2 * i], b = ab[2 * i + 1];
      if (!(a >= 0.0 && a < 1.0 && b >= 0.0 && b < 1.0)) return fail("a coordinate outside [0, 1)");
      if (tri[i] && a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; folded++; if (a + b > 1.0) outside++; }
      for (int c = 0; c < 3; ++c) {
        const double want = (quv[9 * i + c] + quv[9 * i + 3 + c] * a) + quv[9 * i + 6 + c] * b;
        if (std::memcmp(&want, &T[3 * i + c], 8)) return fail("the aim differs from its own arithmetic");
      }
    }
  }
  if (outside) return fail("a folded point outside its triangle");
  // the validation
  {
    std::vector<float> emit(3 * 64, 0.0f);
    uint32_t count = 0;
    emit[3 * 9 + 1] = 0.5f; emit[3 * 40] = 1.0f;
    if (fl_emit_check(emit.data(), 64, &count) != 64u || count != 2u) return fail("emit_check on a good table");
    emit[3 * 50 + 2] = NAN; emit[3 * 20] = 1.5f;
    if (fl_emit_check(emit.data(), 64, &count) != 20u) return fail("emit_check: the lowest bad entry");
  }
  // the loader and the writer: all four forms, both point forms; load -> write -> load is bit for bit
  const char* text =
      "{\"width\":12,\"height\":8,\"samples_per_pixel\":2,\"max_depth\":4,\"sky\":null,"
      "\"camera\":{\"look_from\":{\"x\":0.5,\"y\":0.5,\"z\":6},\"look_at\":{\"x\":0.5,\"y\":0.5,\"z\":0},\"vup\":{\"x\":0,\"y\":1,\"z\":0},\"vfov\":40,\"aspect\":1.5},"
      "\"objects\":[{\"q\":[0,0,0],\"u\":[1,0,0],\"v\":[0,1,0],\"emit\":[1.0,0.9,0.75],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"triangle\":[[0,0,1],[1,0,1],[0,1,1]],\"emit\":{\"x\":0.1,\"y\":0.2,\"z\":0.3},\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"box\":{\"min\":[1,1,1],\"max\":[2,2,2]},\"emit\":[0,0,0],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"mesh\":{\"vertices\":[[0,0,2],[1,0,2],[0,1,2],[1,1,2]],\"faces\":[[0,1,2],[1,3,2]]},\"emit\":[0,0,0.5],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"center\":[0.5,0.5,-3],\"radius\":1.0,\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},"
      "{\"q\":[-3,-1,-3],\"u\":[8,0,0],\"v\":[0,0,8],\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}}]}";
  RtSceneFile *a = nullptr, *b = nullptr;
  if (rt_scene_load_string(text, std::strlen(text), &a) != RT_OK) return fail(rt_host_last_error());
  uint32_t na = 0, nb = 0, nq = 0;
  const float* ea = rt_scene_flat_emit(a, &na);
  if (!ea || na != 11u) return fail("rt_scene_flat_emit: expected 11 entries");
  size_t need = 0;
  rt_scene_to_json(a, nullptr, 0, &need);
  std::vector<char> buf(need);
  if (rt_scene_to_json(a, buf.data(), need, nullptr) != RT_OK) return fail("rt_scene_to_json");
  if (rt_scene_load_string(buf.data(), std::strlen(buf.data()), &b) != RT_OK) return fail(rt_host_last_error());
  const float* eb = rt_scene_flat_emit(b, &nb);
  if (!eb || nb != na || std::memcmp(ea, eb, 12 * (size_t)na)) return fail("the round trip changed the emission");
  // a lit frame of the lane code over the file's world: four emitters, scan and structure
  const RtQuad* quads = rt_scene_quads(a, &nq);
  const RtScene* sc = rt_scene_get(a);
  std::vector<uint8_t> rgb[2];
  std::vector<float> lin[2];
  uint64_t segs[2] = {0, 0};
  for (int bvh = 0; bvh < 2; ++bvh) {
    uint32_t info[3];
    rgb[bvh].resize((size_t)sc->width * sc->height * 3); lin[bvh].resize(rgb[bvh].size());
    if (fl_render(sc, nullptr, quads, nq, nullptr, ea, bvh, rgb[bvh].data(), lin[bvh].data(), &segs[bvh], info)) return fail("fl_render");
    if (info[1] != 4u || info[2] != 4u || !(info[0] & FLAT_LIGHTS_BIT)) return fail("four emitters expected");
  }
  if (segs[0] != segs[1] || std::memcmp(lin[0].data(), lin[1].data(), lin[0].size() * 4)) return fail("the structure's frame differs from the scan's");
  rt_scene_free(a); rt_scene_free(b);
  std::printf("flat lights: %llu folded aims, none outside; round trip of %u entries; a frame of %llu segments with 4 emitters, structure == scan\n",
              (unsigned long long)folded, na, (unsigned long long)segs[0]);
  return 0;
}
