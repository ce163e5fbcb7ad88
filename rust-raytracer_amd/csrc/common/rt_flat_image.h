// rt_flat_image.h — images on flat primitives, compiled by the host (rt_hip_api.hip, scene.cpp, the tests), the device
// (rt_core.h, rt_flat_build.hip) and the CPU tests (tests/flatimage/).  Its bits are the contract; tests/flat_image_mini.py restates it in
// plain Python floats.  Every operation below is ONE IEEE f64 operation in the order written, no contraction; dot and cross are rt_quad.h's.
//
// Once per entry (rt_flat_image_prepare).  The caller gives an RtFlatImage (rt_abi.h): (s, t) at Q, at Q + u and at Q + v, a texture id, two
// wrap modes.  tex_id == RT_FLAT_IMAGE_NONE: "no image", the record is 64 zero bytes.  Otherwise the entry is refused when
//     a uv component is not finite; tex_id >= n_textures; the texture has nbytes != 3 W H, W == 0 or H == 0 (W, H: the DECODED size), or
//     lies outside the 2^31 texels the scene expands to 4-byte texels; a wrap value is above 1; reserved != 0; the entry's own material is
//     not Lambertian or Metal
// and the record is {u32 texel_off, W, H, wrap_s | wrap_t << 1; f64 uv[6]}: 64 B per entry, indexed by entry k.  W == 0 says "no image":
// the first 16 bytes decide.
// Per accepted hit of entry k (rt_flat_image_texel), at shading only.  P = o + d t as the test formed it, O the entry's origin at the
// sample's shutter time (Q of a still entry), u, v, w the entry's record's:
//     p = P - O    alpha = dot(w, cross(p, v))    beta = dot(w, cross(u, p))          (rt_flat_normal.h rt_flat_barycentric: the same code)
//     gamma = (1 - alpha) - beta
//     s = (s0 gamma + s1 alpha) + s2 beta        t = (t0 gamma + t1 alpha) + t2 beta   (one formula for both shapes: past the diagonal of a
//                                                                                        parallelogram gamma < 0, the affine extension)
//     wrap, per axis:   REPEAT  x' = x - floor(x);  !(x' < 1.0): x' = 0.0            (x = -tiny rounds to 1; a NaN or an infinity gives 0)
//                       CLAMP   x' = fmin(fmax(x, 0.0), 1.0), a NaN: 0.0
//     col = min((u32)floor(s' W), W - 1)         row = min((u32)floor((1.0 - t') H), H - 1)      (row 0 is the top: t points up)
//     index = texel_off + row W + col            the colour: rgb_of_texel(tex4[index]) — bytes / 255 through rt_div255f (rt_core.h)
// Nearest texel only.  s', t' are in [0, 1], so col < W and row < H always: no index leaves the texture.
#pragma once
#include "../../../include/rt_abi.h"
#include "rt_flat_normal.h"

// the resident record (rt_hip_scene_table "flat_images")
struct RtFlatImageRec {
  uint32_t texel_off, W, H, wrap;  // W == 0: no image; wrap = wrap_s | wrap_t << 1
  double uv[6];
};
// what prepare knows of texture i of the scene: its first texel in DevScene::tex4 and its decoded size; ok = RT_FLAT_IMAGE_TEX_OK or why not
struct RtFlatImageTex { uint32_t texel_off, W, H, ok; };
enum { RT_FLAT_IMAGE_TEX_OK = 1, RT_FLAT_IMAGE_TEX_SIZE = 2, RT_FLAT_IMAGE_TEX_FAR = 3 };

// texture i of a scene's table; `before`: the texels of textures 0 .. i - 1 (build_texels lays them out back to back, 2^31 at the most)
RT_QUAD_FN RtFlatImageTex rt_flat_image_tex(uint32_t width, uint32_t height, uint64_t nbytes, uint64_t before) {
  RtFlatImageTex t = {0u, width, height, RT_FLAT_IMAGE_TEX_OK};
  const uint64_t n_px = (uint64_t)width * (uint64_t)height;
  if (width == 0u || height == 0u || nbytes != 3u * n_px) t.ok = RT_FLAT_IMAGE_TEX_SIZE;
  else if (before + nbytes / 3u >= (1ull << 31)) t.ok = RT_FLAT_IMAGE_TEX_FAR;
  else t.texel_off = (uint32_t)before;
  return t;
}

enum {  // rt_flat_image_prepare
  RT_FLAT_IMAGE_ABSENT = 0, RT_FLAT_IMAGE_PRESENT = 1,
  RT_FLAT_IMAGE_BAD_UV = 2, RT_FLAT_IMAGE_BAD_TEX_ID = 3, RT_FLAT_IMAGE_BAD_TEX_SIZE = 4, RT_FLAT_IMAGE_BAD_TEX_FAR = 5,
  RT_FLAT_IMAGE_BAD_WRAP = 6, RT_FLAT_IMAGE_BAD_RESERVED = 7, RT_FLAT_IMAGE_BAD_MATERIAL = 8
};
RT_QUAD_FN const char* rt_flat_image_why(int code) {
  switch (code) {
    case RT_FLAT_IMAGE_BAD_UV: return "every uv component must be finite";
    case RT_FLAT_IMAGE_BAD_TEX_ID: return "tex_id lies outside the scene's textures";
    case RT_FLAT_IMAGE_BAD_TEX_SIZE: return "the texture's nbytes must be 3 x width x height, with neither side zero";
    case RT_FLAT_IMAGE_BAD_TEX_FAR: return "the texture lies outside the 2^31 texels the scene keeps as 4-byte texels";
    case RT_FLAT_IMAGE_BAD_WRAP: return "wrap must be RT_WRAP_REPEAT (0) or RT_WRAP_CLAMP (1)";
    case RT_FLAT_IMAGE_BAD_RESERVED: return "reserved must be 0";
    case RT_FLAT_IMAGE_BAD_MATERIAL: return "an image needs a Lambertian or Metal entry";
    default: return "";
  }
}

// `kind`: the entry's own material (RT_MAT_*); tex: the scene's n_textures textures.  *out is written for ABSENT and PRESENT only.
RT_QUAD_FN int rt_flat_image_prepare(const RtFlatImage& in, const RtFlatImageTex* tex, uint32_t n_textures, uint32_t kind, RtFlatImageRec* out) {
  if (in.tex_id == RT_FLAT_IMAGE_NONE) {
    out->texel_off = out->W = out->H = out->wrap = 0u;
    for (int k = 0; k < 6; ++k) out->uv[k] = 0.0;
    return RT_FLAT_IMAGE_ABSENT;
  }
  for (int k = 0; k < 6; ++k)
    if (!rt_quad_finite(in.uv[k])) return RT_FLAT_IMAGE_BAD_UV;
  if (in.tex_id >= n_textures) return RT_FLAT_IMAGE_BAD_TEX_ID;
  const RtFlatImageTex t = tex[in.tex_id];
  if (t.ok == RT_FLAT_IMAGE_TEX_FAR) return RT_FLAT_IMAGE_BAD_TEX_FAR;
  if (t.ok != RT_FLAT_IMAGE_TEX_OK) return RT_FLAT_IMAGE_BAD_TEX_SIZE;
  if (in.wrap_s > 1u || in.wrap_t > 1u) return RT_FLAT_IMAGE_BAD_WRAP;
  if (in.reserved != 0u) return RT_FLAT_IMAGE_BAD_RESERVED;
  if (kind != RT_MAT_LAMBERTIAN && kind != RT_MAT_METAL) return RT_FLAT_IMAGE_BAD_MATERIAL;
  out->texel_off = t.texel_off; out->W = t.W; out->H = t.H; out->wrap = in.wrap_s | (in.wrap_t << 1);
  for (int k = 0; k < 6; ++k) out->uv[k] = in.uv[k];
  return RT_FLAT_IMAGE_PRESENT;
}

RT_QUAD_FN bool rt_flat_image_present(const RtFlatImageRec& rec) { return rec.W != 0u; }

RT_QUAD_FN double rt_flat_image_wrap(double x, uint32_t clamp) {
  if (clamp) {
    if (x != x) return 0.0;
    return fmin(fmax(x, 0.0), 1.0);
  }
  double f = x - floor(x);
  if (!(f < 1.0)) f = 0.0;
  return f;
}

struct RtFlatImageTexel { uint32_t col, row, index; };
// The texel of a hit at P on an entry with frame u, v, w whose origin, at the sample's shutter time, is O; rec: a record that has an image.
RT_QUAD_FN RtFlatImageTexel rt_flat_image_texel(const RtFlatImageRec& rec, const double O[3], const double u[3], const double v[3], const double w[3],
                                                const double P[3]) {
  double p[3], alpha, beta;
  for (int k = 0; k < 3; ++k) p[k] = P[k] - O[k];
  rt_flat_barycentric(u, v, w, p, &alpha, &beta);
  const double gamma = (1.0 - alpha) - beta;
  const double s = (rec.uv[0] * gamma + rec.uv[2] * alpha) + rec.uv[4] * beta;
  const double t = (rec.uv[1] * gamma + rec.uv[3] * alpha) + rec.uv[5] * beta;
  const double sw = rt_flat_image_wrap(s, rec.wrap & 1u), tw = rt_flat_image_wrap(t, (rec.wrap >> 1) & 1u);
  RtFlatImageTexel x;
  x.col = (uint32_t)floor(sw * (double)rec.W);
  if (x.col > rec.W - 1u) x.col = rec.W - 1u;
  x.row = (uint32_t)floor((1.0 - tw) * (double)rec.H);
  if (x.row > rec.H - 1u) x.row = rec.H - 1u;
  x.index = rec.texel_off + x.row * rec.W + x.col;
  return x;
}
