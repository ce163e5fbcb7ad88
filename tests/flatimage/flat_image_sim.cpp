// flat_image_sim.cpp — TEST TOOL, not part of the product.  Images on flat primitives built for the host: the header
// (csrc/common/rt_flat_image.h) on tables of hits, and the QUADS lane code of tests/lanesim/lane_sim.h on a world bound as
// rt_hip_scene_set_flat_images leaves it on the device — the records behind a header that names the image table and the 4-byte texels,
// FLAT_IMAGES_BIT — beside shading normals (§25), motion (§27) and emission (§28) bound as their own calls leave them.
// tests/flat_image_sim.py builds and binds it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-raytracer_amd/csrc/hip/rt_tables.h"
// tests/lanesim/lane_sim.h — not to be edited — restates the kernels' QUADS arm with the call they made before the structure; in THIS build
// that call is the kernels' own (as in tests/flatmotion/flat_motion_sim.cpp)
#define quads_hit(o, d, view, n, base, closest, best) flats_hit(ds, tb, o, d, closest, best)
#include "../lanesim/lane_sim.h"
#undef quads_hit

using namespace lanesim;

namespace {
std::vector<RtFlatImageTex> tex_table(const RtScene& sc) {
  std::vector<RtFlatImageTex> table(sc.n_textures);
  uint64_t before = 0;
  for (uint32_t i = 0; i < sc.n_textures; ++i) {
    const RtTexture& x = sc.textures[i];
    table[i] = rt_flat_image_tex(x.width, x.height, x.nbytes, before);
    before = (table[i].ok == RT_FLAT_IMAGE_TEX_FAR || before + x.nbytes / 3 >= (1ull << 31)) ? (1ull << 31) : before + x.nbytes / 3;
  }
  return table;
}
struct ImageWorld {
  World w;
  std::vector<double> normals, still;
  std::vector<RtQuadRec> blob;
  std::vector<uint32_t> lights;
  std::vector<RtFlatImageRec> images;
};
// info = {DevScene::n_tris, entries with an image, the lowest refused entry or 0xFFFFFFFF, its reason}.  1: the world is refused; 2: a bad emit;
// 3: bad normals; 4: a bad displacement; 5: a refused image (info[2], info[3])
int build_world(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const double* move, const float* emit,
                const RtFlatImage* images, int flat_bvh, ImageWorld& s, uint32_t* info) {
  World& w = s.w;
  info[0] = info[1] = info[3] = 0; info[2] = 0xFFFFFFFFu;
  if (!sc || !n_quads || !build_tables(*sc, w.t, false, center1, quads, n_quads).empty()) return 1;
  uint32_t moving = 0;
  if (move) {
    w.t.flat_motion.assign(4 * (size_t)n_quads, 0.0);
    for (uint32_t k = 0; k < n_quads; ++k) {
      const int kind = rt_flat_motion_prepare(w.t.quads[k], move + 3 * (size_t)k, &w.t.flat_motion[4 * (size_t)k]);
      if (kind == RT_FLAT_MOTION_BAD) return 4;
      moving += kind == RT_FLAT_MOTION_MOVING;
    }
    if (!moving) w.t.flat_motion.clear();
  }
  if (flat_bvh && !build_flat_bvh(w.t).empty()) return 1;
  build_texels(*sc, w.t);
  fill_dev_scene(*sc, w.t, w.ds);
  bind_host_tables(w.t, w.ds);
  uint32_t smooth = 0;
  if (normals) {
    s.normals.assign(9 * (size_t)n_quads, 0.0);
    for (uint32_t k = 0; k < n_quads; ++k) {
      const int kind = rt_flat_normal_prepare(normals + 9 * (size_t)k, &s.normals[9 * (size_t)k]);
      if (kind == RT_FLAT_NORMAL_BAD) return 3;
      smooth += kind == RT_FLAT_NORMAL_SMOOTH;
    }
  }
  uint32_t present = 0;
  if (images) {
    const std::vector<RtFlatImageTex> table = tex_table(*sc);
    s.images.resize(n_quads);
    for (uint32_t k = 0; k < n_quads; ++k) {
      const int code = rt_flat_image_prepare(images[k], table.data(), sc->n_textures, quads[k].kind, &s.images[k]);
      if (code > RT_FLAT_IMAGE_PRESENT) { info[2] = k; info[3] = (uint32_t)code; return 5; }
      present += code == RT_FLAT_IMAGE_PRESENT;
    }
  }
  if (moving || smooth || present) {
    FlatBvhHeader* h;
    if (w.ds.n_tris & FLAT_BVH_BIT) h = const_cast<FlatBvhHeader*>(reinterpret_cast<const FlatBvhHeader*>(w.ds.quads.rec) - 1);
    else {
      s.blob.resize((size_t)n_quads + 1);
      std::memcpy(s.blob.data() + 1, w.t.quads.data(), (size_t)n_quads * sizeof(RtQuadRec));
      h = reinterpret_cast<FlatBvhHeader*>(s.blob.data());
      std::memset(h, 0, sizeof *h);
      h->rec = s.blob.data() + 1; h->lim = w.ds.quads.lim; h->n_quads = n_quads; h->id_base = w.ds.n_spheres;
      w.ds.quads.rec = s.blob.data() + 1;
    }
    if (smooth) { h->normals = s.normals.data(); w.ds.n_tris |= FLAT_NORMALS_BIT; }
    if (moving) { h->motion = w.t.flat_motion.data(); w.ds.n_tris |= FLAT_MOTION_BIT; }
    if (present) { h->images = s.images.data(); h->tex4 = w.ds.tex4; w.ds.n_tris |= FLAT_IMAGES_BIT; }
  }
  if (moving && !w.ds.motion) {
    s.still.assign(4 * (size_t)(sc->n_spheres ? sc->n_spheres : 1u), -0.0);
    w.ds.motion = s.still.data();
  }
  uint32_t n_emit = 0;
  if (emit && rt_flat_light_emit_check(emit, n_quads, &n_emit) != n_quads) return 2;
  if (n_emit) {
    const std::vector<SphereMat> flat_mat(w.t.mat.begin() + sc->n_spheres, w.t.mat.end());
    const std::vector<MatCore> flat_matc(w.t.matc.begin() + sc->n_spheres, w.t.matc.end());
    std::vector<SphereMat> mat;
    std::vector<MatCore> matc;
    std::vector<uint32_t> emitters;
    build_flat_lights(flat_mat, flat_matc, w.t.lights, sc->n_spheres, emit, mat, matc, s.lights, emitters);
    std::copy(mat.begin(), mat.end(), w.t.mat.begin() + sc->n_spheres);
    std::copy(matc.begin(), matc.end(), w.t.matc.begin() + sc->n_spheres);
    w.ds.lights = s.lights.data();
    w.ds.n_lights = (uint32_t)s.lights.size();
    w.ds.light_thr[0] = 1.0 - (double)w.ds.n_lights * 0.1;
    w.ds.light_thr[1] = 1.0 - (double)w.ds.n_lights * 0.05;
    w.ds.n_tris |= FLAT_LIGHTS_BIT;
  }
  info[0] = w.ds.n_tris; info[1] = present;
  return 0;
}
#define FI_X8(F) {F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7)}
#define FI_RENDER(k) sim_render<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
#define FI_AOVS(k) sim_aovs<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0, true>
uint64_t (*const RENDER[8])(const RtScene&, const DevScene&, uint8_t*, float*) = FI_X8(FI_RENDER);   // bit 2: HL
void (*const AOVS[8])(const RtScene&, const DevScene&, uint32_t, float*) = FI_X8(FI_AOVS);          // bit 2: MOTION
// tests/lanesim/lane_sim.h's sim_render with the thin lens of DESIGN.md §13 (as tests/flatlight/flat_light_sim.cpp: that loop is the
// pinhole camera's alone and is not to be edited)
template <bool HL, bool MEDIUM, bool SOLID>
uint64_t lens_render(const RtScene& sc, const DevScene& ds, uint8_t* rgb8, float* linear) {
  uint64_t segs = 0;
  for (uint32_t y = 0; y < sc.height; ++y)
    for (uint32_t x = 0; x < sc.width; ++x) {
      Lane<HL, false> L;
      std::memset(&L, 0, sizeof L);
      LightStack<HL> light_stack;
      LightParked light_parked;
      lane_attach_light_state(L, light_stack, &light_parked);
      L.ra.pixel = y * sc.width + x; L.ra.k0 = ds.seed_lo; L.ra.k1 = ds.seed_hi;
      unsigned long long facc[3] = {0ull, 0ull, 0ull};
      for (L.s = 0; L.s < sc.samples_per_pixel && sc.max_depth != 0; ++L.s) {
        lane_begin_sample<true>(ds, L, x, y);
        const float tau = ds.motion ? sample_time(L.ra) : 0.0f;
        for (;;) {
          L.n_segments++;
          const int st = with_tables(ds, tau, [&](const auto& tb) {
            double closest = T_MAX;
            int best = -1;
            uint32_t ns = 0;
            const MediumCtx mc{ds.medium, L.ra, L.node};
            hit_world_grid<MEDIUM>(ds, tb, L.o, L.d, closest, best, L.n_exact, ns, &mc);
            const HitCB r = flats_hit(ds, tb, L.o, L.d, closest, best);
            return lane_shade<MEDIUM, SOLID, true>(ds, tb, L, r.best, r.closest);
          });
          if (st == LANE_FINISHED) break;
        }
        for (int k = 0; k < 3; ++k) facc[k] += sample_to_fixed(L.val[k]);
      }
      for (int k = 0; k < 3; ++k) {
        const float lin = fixed_to_mean(facc[k], sc.samples_per_pixel);
        const size_t o = ((size_t)y * sc.width + x) * 3 + k;
        linear[o] = lin;
        rgb8[o] = f32_to_u8(sqrtf(lin));
      }
      segs += L.n_segments;
    }
  return segs;
}
#define FI_LENS(k) lens_render<((k) & 4) != 0, ((k) & F_MEDIUM) != 0, ((k) & F_SOLID) != 0>
uint64_t (*const RENDER_LENS[8])(const RtScene&, const DevScene&, uint8_t*, float*) = FI_X8(FI_LENS);   // bit 2: HL
}  // namespace

// rt_flat_image_texel of n hits: rec[n] (64 B records, W > 0), ouvw[n][12] (O, u, v, w), P[n][3] -> texel[n][3] = {col, row, index}
extern "C" void fi_texel(const void* rec, const double* ouvw, const double* P, uint64_t n, uint32_t* texel) {
  const RtFlatImageRec* r = static_cast<const RtFlatImageRec*>(rec);
  for (uint64_t i = 0; i < n; ++i) {
    const double* f = ouvw + 12 * i;
    const RtFlatImageTexel x = rt_flat_image_texel(r[i], f, f + 3, f + 6, f + 9, P + 3 * i);
    texel[3 * i] = x.col; texel[3 * i + 1] = x.row; texel[3 * i + 2] = x.index;
  }
}
// rgb_of_texel of n 4-byte texels -> rgb[n][3] f32
extern "C" void fi_colour(const uint32_t* words, uint64_t n, float* out) {
  for (uint64_t i = 0; i < n; ++i) { const Rgb c = rgb_of_texel(words[i]); out[3 * i] = c.r; out[3 * i + 1] = c.g; out[3 * i + 2] = c.b; }
}
// the cold function itself on a table of its own: one entry {rec, frame} and the texels tex4 -> rgb[n][3] f32 (negative red: no image)
extern "C" void fi_albedo(const void* rec, const double* quv, const uint32_t* tex4, const double* origin, const double* P, uint64_t n, float* out) {
  RtQuadRec blob[2];
  std::memset(blob, 0, sizeof blob);
  if (rt_quad_prepare(quv, quv + 3, quv + 6, &blob[1])) return;
  FlatBvhHeader* h = reinterpret_cast<FlatBvhHeader*>(&blob[0]);
  h->rec = &blob[1]; h->n_quads = 1; h->images = static_cast<const RtFlatImageRec*>(rec); h->tex4 = tex4;
  for (uint64_t i = 0; i < n; ++i) {
    const Rgb c = flat_image_albedo(h, 0u, v3(origin[3 * i], origin[3 * i + 1], origin[3 * i + 2]), v3(P[3 * i], P[3 * i + 1], P[3 * i + 2]));
    out[3 * i] = c.r; out[3 * i + 1] = c.g; out[3 * i + 2] = c.b;
  }
}
// the scene's texture table as rt_hip_scene_set_flat_images' prepare kernel reads it: out[n_textures][4]
extern "C" void fi_tex_table(const RtScene* sc, uint32_t* out) {
  const std::vector<RtFlatImageTex> t = tex_table(*sc);
  if (!t.empty()) std::memcpy(out, t.data(), t.size() * sizeof(RtFlatImageTex));
}
// the host path: rt_flat_image_prepare of every entry -> out (64 B records, untouched where refused), code[k]
extern "C" void fi_prepare(const RtFlatImage* in, uint32_t n, const void* tex, uint32_t n_textures, const uint32_t* kind, void* out, int32_t* code) {
  RtFlatImageRec* o = static_cast<RtFlatImageRec*>(out);
  for (uint32_t k = 0; k < n; ++k) {
    RtFlatImageRec rec;
    code[k] = rt_flat_image_prepare(in[k], static_cast<const RtFlatImageTex*>(tex), n_textures, kind[k], &rec);
    if (code[k] <= RT_FLAT_IMAGE_PRESENT) o[k] = rec;
  }
}

// The frame of the QUADS lane code.  normals: null or n x 9; move: null or n x 3; emit: null or n x 3; images: null or n; lens: null or
// {u[3], v[3], radius} with the camera of `sc` already on the focus plane.
extern "C" int fi_render(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const double* move,
                         const float* emit, const RtFlatImage* images, int flat_bvh, const double* lens, uint8_t* rgb8, float* linear, uint64_t* segments,
                         uint32_t* info) {
  ImageWorld s;
  if (const int rc = build_world(sc, center1, quads, n_quads, normals, move, emit, images, flat_bvh, s, info)) return rc;
  const uint32_t key = (s.w.ds.n_lights ? 4u : 0u) | (features(s.w) & 3u);
  if (lens) {
    for (int k = 0; k < 3; ++k) { s.w.ds.lens_u[k] = lens[k]; s.w.ds.lens_v[k] = lens[3 + k]; }
    s.w.ds.lens_r = lens[6];
    *segments = RENDER_LENS[key](*sc, s.w.ds, rgb8, linear);
  } else *segments = RENDER[key](*sc, s.w.ds, rgb8, linear);
  return 0;
}
// The first-hit records of n samples per pixel (height x width x 8 f32).
extern "C" int fi_aovs(const RtScene* sc, const double* center1, const RtQuad* quads, uint32_t n_quads, const double* normals, const double* move,
                       const float* emit, const RtFlatImage* images, int flat_bvh, uint32_t n, float* out) {
  ImageWorld s;
  uint32_t info[4];
  if (const int rc = build_world(sc, center1, quads, n_quads, normals, move, emit, images, flat_bvh, s, info)) return rc;
  AOVS[(s.w.ds.motion ? 4u : 0u) | (features(s.w) & 3u)](*sc, s.w.ds, n, out);
  return 0;
}
