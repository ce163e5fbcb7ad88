// fuzz_normals.cpp — development tool: the host code of shading normals under ASan/UBSan.  Random and hostile vertex
// normals through rt_flat_normal_prepare and rt_flat_normal_shade (csrc/common/rt_flat_normal.h), and meshes with "normals" / "smooth"
// through rt_scene_load_string, rt_scene_flat_normals and rt_scene_to_json: the written text must load to the same quads and normals.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/fuzz/fuzz_normals.cpp rust-raytracer_amd/csrc/host/scene.cpp \
//       rust-raytracer_amd/csrc/host/jpeg.cpp -Iinclude -lz -lpthread -o /tmp/fuzz_normals && /tmp/fuzz_normals <seed> <iterations>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>
#include "../../include/rt_abi.h"
#include "../../rust-raytracer_amd/csrc/common/rt_flat_normal.h"

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? atoll(argv[1]) : 1);
  const int iters = argc > 2 ? atoi(argv[2]) : 200;
  auto U = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 11) * 0x1p-53; };
  const double odd[] = {0.0, -0.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                        5e-324, 1e-160, 1e160, 1e308};
  auto value = [&]() { return rng() % 8 == 0 ? odd[rng() % 9] : U(-2, 2) * std::pow(10.0, rng() % 4 == 0 ? U(-150, 150) : 0.0); };
  long shaded = 0, fell[3] = {0, 0, 0}, refused = 0, round_trips = 0, load_errors = 0;
  for (int it = 0; it < iters; ++it) {
    // 1. the header
    for (int k = 0; k < 500; ++k) {
      double quv[9], in[9], rec[9], d[3], P[3], n[3];
      for (double& x : quv) x = U(-3, 3);
      for (double& x : in) x = value();
      for (double& x : d) x = value();
      for (double& x : P) x = value();
      RtQuadRec r;
      if (rt_quad_prepare(quv, quv + 3, quv + 6, &r)) continue;
      const int kind = rt_flat_normal_prepare(in, rec);
      if (kind == RT_FLAT_NORMAL_BAD) { refused++; std::memcpy(rec, in, sizeof rec); }   // (a refused record still goes through shade)
      const int f = rt_flat_normal_shade(r, rec, d, P, n);
      shaded++;
      for (int b = 0; b < 3; ++b) fell[b] += (f >> b) & 1;
      const bool dn = rt_quad_dot(d, n) < 0.0;
      if (kind == RT_FLAT_NORMAL_SMOOTH && std::isfinite(rt_quad_dot(d, r.n)) && rt_quad_dot(d, r.n) != 0.0 && !dn && std::isfinite(rt_quad_dot(d, n))) {
        std::fprintf(stderr, "iteration %d: the normal does not face the incoming ray\n", it);
        return 1;
      }
    }
    // 2. the loader and the writer
    const int nv = 3 + (int)(rng() % 6), nf = 1 + (int)(rng() % 6);
    std::string verts, faces, normals;
    char buf[128];
    for (int i = 0; i < nv; ++i) {
      std::snprintf(buf, sizeof buf, "%s[%.17g,%.17g,%.17g]", i ? "," : "", U(-2, 2), U(-2, 2), U(-2, 2));
      verts += buf;
      const bool hostile = rng() % 16 == 0;
      std::snprintf(buf, sizeof buf, "%s[%.17g,%.17g,%.17g]", i ? "," : "", hostile ? 0.0 : U(-2, 2), hostile ? 0.0 : U(-2, 2), hostile ? (rng() % 2 ? 0.0 : 1e-170) : U(-2, 2));
      normals += buf;
    }
    if (rng() % 8 == 0) normals += ",[0,0,1]";   // one too many
    for (int i = 0; i < nf; ++i) {
      std::snprintf(buf, sizeof buf, "%s[%d,%d,%d]", i ? "," : "", (int)(rng() % nv), (int)(rng() % nv), (int)(rng() % (nv + (rng() % 32 == 0))));
      faces += buf;
    }
    const int mode = (int)(rng() % 4);
    const std::string extra = mode == 0 ? "" : mode == 1 ? ",\"normals\":[" + normals + "]" : mode == 2 ? ",\"smooth\":true" : ",\"smooth\":true,\"normals\":[" + normals + "]";
    const std::string text = "{\"width\":8,\"height\":8,\"samples_per_pixel\":1,\"max_depth\":4,\"sky\":{\"texture\":\"\"},\"camera\":{\"look_from\":[0,0,5],"
                             "\"look_at\":[0,0,0],\"vup\":[0,1,0],\"vfov\":40.0,\"aspect\":1.0},\"objects\":[{\"center\":[0,0,0],\"radius\":0.5,\"material\":"
                             "{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}},{\"mesh\":{\"vertices\":[" + verts + "],\"faces\":[" + faces + "]" + extra +
                             "},\"material\":{\"Metal\":{\"albedo\":[0.9,0.9,0.9],\"fuzz\":0.0}}}]}";
    RtSceneFile* a = nullptr;
    if (rt_scene_load_string(text.c_str(), text.size(), &a) != RT_OK) { load_errors++; continue; }
    uint32_t nq = 0, nn = 0;
    const RtQuad* q = rt_scene_quads(a, &nq);
    const double* nr = rt_scene_flat_normals(a, &nn);
    if ((mode == 1 || mode == 2) && nn != nq) { std::fprintf(stderr, "iteration %d: %u normals for %u entries\n", it, nn, nq); return 1; }
    size_t need = 0;
    (void)rt_scene_to_json(a, nullptr, 0, &need);
    std::vector<char> json_buf(need + 1);
    if (rt_scene_to_json(a, json_buf.data(), json_buf.size(), &need) != RT_OK) { std::fprintf(stderr, "iteration %d: rt_scene_to_json failed\n", it); return 1; }
    const char* json = json_buf.data();
    RtSceneFile* b = nullptr;
    if (rt_scene_load_string(json, std::strlen(json), &b) != RT_OK) { std::fprintf(stderr, "iteration %d: the written scene does not load: %s\n", it, rt_host_last_error()); return 1; }
    uint32_t nq2 = 0, nn2 = 0;
    const RtQuad* q2 = rt_scene_quads(b, &nq2);
    const double* nr2 = rt_scene_flat_normals(b, &nn2);
    if (nq2 != nq || nn2 != nn || std::memcmp(q, q2, nq * sizeof(RtQuad)) || (nn && std::memcmp(nr, nr2, (size_t)nn * 72))) {
      std::fprintf(stderr, "iteration %d: load -> write -> load is not bit for bit\n", it);
      return 1;
    }
    round_trips++;
    rt_scene_free(a);
    rt_scene_free(b);
  }
  std::printf("%ld hits shaded (mm %ld, side %ld, grazing %ld fallbacks; %ld records refused), %ld round trips, %ld load errors\n", shaded, fell[0], fell[1], fell[2],
              refused, round_trips, load_errors);
  return 0;
}
