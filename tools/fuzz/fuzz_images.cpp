// fuzz_images.cpp — development tool: the host code of images on flat primitives under ASan/UBSan.  Random and hostile
// entries through rt_flat_image_prepare and rt_flat_image_texel (csrc/common/rt_flat_image.h) — every index must stay inside its texture —
// and quads, triangles, boxes and meshes with "image" / "uvs" through rt_scene_load_string, rt_scene_flat_images and rt_scene_to_json:
// the written text must load to the same quads and images.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/fuzz/fuzz_images.cpp rust-raytracer_amd/csrc/host/scene.cpp \
//       rust-raytracer_amd/csrc/host/jpeg.cpp -Iinclude -lz -lpthread -o /tmp/fuzz_images && /tmp/fuzz_images <seed> <iterations> <a .jpg> <another>
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
#include "../../rust-raytracer_amd/csrc/common/rt_flat_image.h"

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? atoll(argv[1]) : 1);
  const int iters = argc > 2 ? atoi(argv[2]) : 200;
  const std::string jpg[2] = {argc > 3 ? argv[3] : "scenes/data/earth.jpg", argc > 4 ? argv[4] : "scenes/data/moon.jpg"};
  auto U = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 11) * 0x1p-53; };
  const double odd[] = {0.0, -0.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                        5e-324, -5e-324, 1e-160, 1e160, 1e308, -1e308, 1.0, -1.0};
  auto value = [&]() { return rng() % 8 == 0 ? odd[rng() % 13] : U(-2, 2) * std::pow(10.0, rng() % 4 == 0 ? U(-150, 150) : 0.0); };
  const RtFlatImageTex table[4] = {rt_flat_image_tex(8, 4, 96, 0), rt_flat_image_tex(1, 1, 3, 32), rt_flat_image_tex(7, 0, 0, 33), rt_flat_image_tex(3, 3, 26, 33)};
  long texels = 0, refused[16] = {0}, round_trips = 0, load_errors = 0;
  for (int it = 0; it < iters; ++it) {
    // 1. the header
    for (int k = 0; k < 500; ++k) {
      double quv[9], O[3], P[3];
      for (double& x : quv) x = U(-3, 3);
      for (double& x : O) x = value();
      for (double& x : P) x = value();
      RtQuadRec r;
      if (rt_quad_prepare(quv, quv + 3, quv + 6, &r)) continue;
      RtFlatImage in;
      for (double& x : in.uv) x = rng() % 4 == 0 ? value() : U(-3, 3);
      in.tex_id = rng() % 16 == 0 ? (rng() % 2 ? RT_FLAT_IMAGE_NONE : 9u) : (uint32_t)(rng() % 8 == 0 ? 2 + rng() % 2 : rng() % 2);
      in.wrap_s = (uint32_t)(rng() % 16 == 0 ? 2 : rng() % 2); in.wrap_t = (uint32_t)(rng() % 16 == 0 ? 7 : rng() % 2);
      in.reserved = rng() % 32 == 0;
      RtFlatImageRec rec;
      const int code = rt_flat_image_prepare(in, table, 4, (uint32_t)(rng() % 8 == 0 ? 2 + rng() % 6 : rng() % 2), &rec);
      refused[code & 15]++;
      if (code != RT_FLAT_IMAGE_PRESENT) continue;
      const RtFlatImageTexel x = rt_flat_image_texel(rec, O, r.u, r.v, r.w, P);
      texels++;
      if (x.col >= rec.W || x.row >= rec.H || x.index != rec.texel_off + x.row * rec.W + x.col) {
        std::fprintf(stderr, "iteration %d: texel (%u, %u) index %u leaves a %u x %u texture at %u\n", it, x.col, x.row, x.index, rec.W, rec.H, rec.texel_off);
        return 1;
      }
    }
    // 2. the loader and the writer: a quad, a triangle, a box and a mesh, each with or without an image, sometimes with a mistake
    auto pair = [&](bool hostile) {
      char b[96];
      std::snprintf(b, sizeof b, "[%.17g,%s]", U(-3, 3), hostile ? "1e999" : std::to_string(U(-3, 3)).c_str());
      return std::string(b);
    };
    auto uvs = [&](int n) {
      std::string s = ",\"uvs\":[";
      const int count = rng() % 32 == 0 ? n + 1 : n;
      for (int i = 0; i < count; ++i) s += (i ? "," : "") + pair(rng() % 256 == 0);
      return s + "]";
    };
    auto image = [&]() {
      const char* wraps[] = {"", ",\"wrap\":\"repeat\"", ",\"wrap\":\"clamp\"", ",\"wrap\":[\"clamp\",\"repeat\"]", ",\"wrap\":\"mirror\"", ",\"wrap\":[\"clamp\"]"};
      return ",\"image\":{\"pixels\":\"" + jpg[rng() % 2] + "\"" + wraps[rng() % (rng() % 16 == 0 ? 6 : 4)] + "}";
    };
    const char* mats[] = {"{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}", "{\"Metal\":{\"albedo\":[0.9,0.9,0.9],\"fuzz\":0.1}}", "{\"Glass\":{\"index_of_refraction\":1.5}}"};
    auto mat = [&]() { return std::string(",\"material\":") + mats[rng() % 48 == 0 ? 2 : rng() % 2]; };
    const int nv = 3 + (int)(rng() % 5), nf = 1 + (int)(rng() % 5);
    std::string verts, faces;
    char buf[160];
    for (int i = 0; i < nv; ++i) { std::snprintf(buf, sizeof buf, "%s[%.17g,%.17g,%.17g]", i ? "," : "", U(-2, 2), U(-2, 2), U(-2, 2)); verts += buf; }
    for (int i = 0; i < nf; ++i) {  // (three different vertices: a face is not degenerate by its indices)
      const int a0 = (int)(rng() % nv), b0 = (a0 + 1 + (int)(rng() % (nv - 1))) % nv;
      int c0 = (int)(rng() % nv);
      while (c0 == a0 || c0 == b0) c0 = (c0 + 1) % nv;
      std::snprintf(buf, sizeof buf, "%s[%d,%d,%d]", i ? "," : "", a0, b0, c0);
      faces += buf;
    }
    std::string objs = "{\"center\":[0,0,0],\"radius\":0.5,\"material\":{\"Lambertian\":{\"albedo\":[0.5,0.5,0.5]}}" + std::string(rng() % 32 == 0 ? image() : "") + "}";
    const bool qi = rng() % 2, ti = rng() % 2, bi = rng() % 2, mi = rng() % 2;
    objs += ",{\"q\":[0,0,0],\"u\":[1,0,0.1],\"v\":[0,1,0]" + (qi ? image() : "") + (qi && rng() % 2 ? uvs(3) : (rng() % 32 == 0 ? uvs(3) : "")) + mat() + "}";
    objs += ",{\"triangle\":[[0,0,1],[1,0,1],[0,1,1.5]]" + (ti ? image() + (rng() % 2 ? uvs(3) : "") : "") + mat() + "}";
    objs += ",{\"box\":{\"min\":[2,0,0],\"max\":[3,1,1]}" + (bi ? image() : "") + (rng() % 32 == 0 ? uvs(3) : "") + mat() + "}";
    objs += ",{\"mesh\":{\"vertices\":[" + verts + "],\"faces\":[" + faces + "]" + (mi && rng() % 16 != 0 ? uvs(nv) : "") + "}" + (mi ? image() : "") + mat() + "}";
    const std::string text = "{\"width\":8,\"height\":8,\"samples_per_pixel\":1,\"max_depth\":4,\"sky\":{\"texture\":\"\"},\"camera\":{\"look_from\":[0,0,5],"
                             "\"look_at\":[0,0,0],\"vup\":[0,1,0],\"vfov\":40.0,\"aspect\":1.0},\"objects\":[" + objs + "]}";
    RtSceneFile* a = nullptr;
    if (rt_scene_load_string(text.c_str(), text.size(), &a) != RT_OK) { load_errors++; continue; }
    uint32_t nq = 0, ni = 0;
    const RtQuad* q = rt_scene_quads(a, &nq);
    const RtFlatImage* im = rt_scene_flat_images(a, &ni);
    if ((qi || ti || bi || mi) != (im != nullptr) || (im && ni != nq)) { std::fprintf(stderr, "iteration %d: %u images for %u entries\n", it, ni, nq); return 1; }
    const uint32_t n_tex = rt_scene_get(a)->n_textures;
    for (uint32_t k = 0; k < ni; ++k)
      if (im[k].tex_id != RT_FLAT_IMAGE_NONE && (im[k].tex_id >= n_tex || im[k].wrap_s > 1 || im[k].wrap_t > 1 || im[k].reserved)) {
        std::fprintf(stderr, "iteration %d: entry %u is not what the library takes\n", it, k);
        return 1;
      }
    size_t need = 0;
    (void)rt_scene_to_json(a, nullptr, 0, &need);
    std::vector<char> json_buf(need + 1);
    if (rt_scene_to_json(a, json_buf.data(), json_buf.size(), &need) != RT_OK) { std::fprintf(stderr, "iteration %d: rt_scene_to_json failed\n", it); return 1; }
    const char* json = json_buf.data();
    RtSceneFile* b = nullptr;
    if (rt_scene_load_string(json, std::strlen(json), &b) != RT_OK) { std::fprintf(stderr, "iteration %d: the written scene does not load: %s\n", it, rt_host_last_error()); return 1; }
    uint32_t nq2 = 0, ni2 = 0;
    const RtQuad* q2 = rt_scene_quads(b, &nq2);
    const RtFlatImage* im2 = rt_scene_flat_images(b, &ni2);
    if (nq2 != nq || ni2 != ni || std::memcmp(q, q2, nq * sizeof(RtQuad)) || (ni && std::memcmp(im, im2, (size_t)ni * sizeof(RtFlatImage)))) {
      std::fprintf(stderr, "iteration %d: load -> write -> load is not bit for bit\n", it);
      return 1;
    }
    round_trips++;
    rt_scene_free(a);
    rt_scene_free(b);
  }
  std::printf("%ld texels looked up (refused: uv %ld, tex_id %ld, size %ld, wrap %ld, reserved %ld, material %ld), %ld round trips, %ld load errors\n", texels,
              refused[RT_FLAT_IMAGE_BAD_UV], refused[RT_FLAT_IMAGE_BAD_TEX_ID], refused[RT_FLAT_IMAGE_BAD_TEX_SIZE], refused[RT_FLAT_IMAGE_BAD_WRAP],
              refused[RT_FLAT_IMAGE_BAD_RESERVED], refused[RT_FLAT_IMAGE_BAD_MATERIAL], round_trips, load_errors);
  return 0;
}
