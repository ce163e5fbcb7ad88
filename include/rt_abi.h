/*
 * rt_abi.h — C ABI of the MI355X path-tracer hot path.
 *
 * The reference (dps/rust-raytracer) has NO FFI of its own: the seam this
 * header defines is cut at the rayon closure in
 *   raytracer/src/raytracer.rs:260-262   bands.into_par_iter().for_each(render_line)
 * Inputs of that closure are the immutable `Config` (raytracer/src/config.rs:66-75)
 * and the light list (`find_lights`, raytracer.rs:220-229); its output is the
 * `pixels: Vec<u8>` framebuffer (raytracer.rs:254), row-major, top row first, RGB8.
 * Everything in this file is plain C: pointers, sizes, POD structs.  No torch /
 * HIP types appear in signatures (streams and device pointers travel as void*).
 *
 * Two product libraries implement it (the CPU checker under oracle/ reuses the structs
 * below but is test infrastructure and is never linked into either):
 *   librt_host.so  (C++, product)   scene JSON/JPEG/PNG/camera — the host plumbing
 *                                   that stays on the CPU (main.rs, config.rs, camera.rs)
 *   librt_hip.so   (HIP,  product)  the gfx950 megakernel = render_line/ray_color/hit_world
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 5u /* v5: RtGroupInfo.transport_fallback, RtGroupRank + rt_hip_group_ranks, rt_hip_group_fallback_reason; the device probes and
                           * debug calls moved to rt_abi_test.h (librt_hip_probe.so); v4: RtStats.group_us, rt_hip_group_submit / _collect;
                           * v3: RtScene.n_gpus, RtStats.{segments_discarded, n_gpus_used, gather_ms, setup_ms}, rt_abi_sizeof */

/* Nested light-ray recursion (raytracer.rs:103-110 calls ray_color(.., 2, 1), which can
 * itself trigger light sampling again) is unbounded in the reference.  Oracle and kernel
 * both stop spawning new light rays below this nesting level (level 0 = camera path). */
#define RT_MAX_LIGHT_NEST 8u

/* ---- error codes (the reference panics; a C ABI returns codes instead) ---- */
enum {
  RT_OK = 0,
  RT_ERR_INVALID = -1,   /* null pointer / inconsistent scene                      */
  RT_ERR_NO_DEVICE = -2, /* no gfx950 device visible                               */
  RT_ERR_HIP = -3,       /* a HIP runtime call failed (see rt_hip_last_error)      */
  RT_ERR_IO = -4,        /* main.rs:14 "Unable to read config file."               */
  RT_ERR_PARSE = -5,     /* main.rs:15 "Unable to parse config json"               */
  RT_ERR_TEXTURE = -6,   /* materials.rs:214-217 / config.rs:37-40 texture failure */
  RT_ERR_PNG = -7,       /* raytracer.rs:265 "error writing image"                 */
  RT_ERR_UNSUPPORTED = -8
};

/* materials.rs:35-42  enum Material, in declaration order */
enum {
  RT_MAT_LAMBERTIAN = 0,
  RT_MAT_METAL = 1,
  RT_MAT_GLASS = 2,
  RT_MAT_TEXTURE = 3,
  RT_MAT_LIGHT = 4,
  /* Participating medium (an extension of the schema; NOT a variant of the reference's enum, whose loader rejects it):
   * a sphere of constant-density fog or smoke.  RtSphere.albedo is its albedo, RtSphere.fuzz_or_ior its density (finite, > 0); the radius
   * must be finite and > 0. */
  RT_MAT_MEDIUM = 5,
  /* Solid textures (extensions of the schema; the reference's loader rejects both).  Both scatter exactly like
   * Lambertian; only the attenuation differs (the contract is below, at rt_hip_scene_create_moving).
   * Checker: RtSphere.albedo is the `even` colour, h_offset the scale (cells per unit length; finite, > 0), and the `odd` colour
   * travels as f32 bit patterns: tex_w = bits(r) | bits(g) << 32, tex_h = bits(b) (the high half of tex_h is ignored). */
  RT_MAT_CHECKER = 6,
  /* Noise: RtSphere.albedo is the colour, h_offset the scale (finite, > 0), tex_id the mode (0 noise, 1 turbulence, 2 marble),
   * tex_w the octaves (1..16; mode 0 ignores their value), tex_h the seed (at most 2^32 - 1). */
  RT_MAT_NOISE = 7
};

/* config.rs:22-28, 49-64: sky null -> black; {"texture":""} -> gradient; path -> texture */
enum { RT_SKY_NONE = 0, RT_SKY_GRADIENT = 1, RT_SKY_TEXTURE = 2 };

/* sphere.rs:18-23 + the material payloads (materials.rs:71-76, 97-103, 131-134, 201-211).
 * Spheres are kept in JSON object order: closest-hit ties (raytracer.rs:52-57) and the
 * light order (raytracer.rs:220-229) follow it. */
typedef struct RtSphere {
  double center[3];
  double radius;      /* may be negative: hollow glass, test_scene.json:137 */
  double fuzz_or_ior; /* Metal.fuzz | Glass.index_of_refraction | Medium.density */
  double h_offset;    /* Texture.h_offset | Checker.scale | Noise.scale      */
  uint64_t tex_w;     /* Texture.width / height AS WRITTEN IN THE JSON      */
  uint64_t tex_h;     /*   (materials.rs:206-210), not the decoded size     */
  float albedo[3];    /* Lambertian/Metal/Medium albedo; ignored for Texture */
  uint32_t kind;      /* RT_MAT_*                                           */
  uint32_t tex_id;    /* index into RtScene.textures when kind==TEXTURE; Noise: the mode */
  uint32_t reserved;
} RtSphere;

/* A quad (an extension of the schema; the reference has no such object and its loader rejects the file): the flat
 * parallelogram q + a u + b v, 0 <= a, b <= 1, two-sided.  The material fields mean what they mean in RtSphere; a quad may be
 * Lambertian, Metal, Glass, Checker or Noise (the solid's pattern in the quad's frame: centre = q).  Texture, Light and Medium quads
 * are RT_ERR_INVALID: a picture comes in beside the material (rt_hip_scene_set_flat_images), a medium needs a volume, and a quad cannot be a Light MATERIAL (emission:
 * rt_hip_scene_set_flat_lights).  Quads do not move within a frame (no center1) unless rt_hip_scene_set_flat_motion gives them a displacement over the shutter; rt_hip_scene_update_flats moves them between frames.
 * Triangles: `reserved` carries the SHAPE of the flat primitive, RT_QUAD_SHAPE_PARALLELOGRAM (0, the quad above) or
 * RT_QUAD_SHAPE_TRIANGLE (1): the points q + a u + b v with 0 <= a, 0 <= b, a + b <= 1, two-sided.  Everything else about the entry —
 * its place in the order, its id, its materials, the refusals — is a quad's.  A value above 1 is RT_ERR_INVALID (`quad k: bad shape`). */
#define RT_QUAD_SHAPE_PARALLELOGRAM 0u
#define RT_QUAD_SHAPE_TRIANGLE 1u
typedef struct RtQuad {
  double q[3], u[3], v[3];
  double fuzz_or_ior;
  double h_offset;
  uint64_t tex_w;
  uint64_t tex_h;
  float albedo[3];
  uint32_t kind;
  uint32_t tex_id;
  uint32_t reserved;  /* the shape: RT_QUAD_SHAPE_* */
} RtQuad;
/* The most quads (of both shapes together) a scene may hold; more is RT_ERR_UNSUPPORTED.  There is no spatial structure over the quads: EVERY ray segment tests
 * EVERY quad, so the cost of a segment is linear in their number. */
#define RT_MAX_QUADS 1024u
/* The most flat primitives of a scene WITH the structure of DESIGN.md §22 (rt_hip_scene_create_flats_bvh; "flat_bvh": true in a scene file):
 * 2^20.  Every place an object id n_spheres + k is kept holds it: `best` is an int32 and quads never go with wide tables, so an id stays below
 * 65 535 + 2^20; the surface record's id is a u32 whose only reserved value is 0xFFFFFFFF; the AOVs and the colour map keep no id. */
#define RT_MAX_FLATS_BVH 1048576u

/* decoded texture pixels, RGB8 (materials.rs:213-219) */
typedef struct RtTexture {
  const uint8_t* rgb8;
  uint64_t nbytes;
  uint32_t width, height; /* decoded size, informational */
} RtTexture;

/* An image on a flat primitive (rt_hip_scene_set_flat_images): entry k of the table belongs to flat primitive k.  uv: the
 * texture coordinates (s, t) at Q, at Q + u and at Q + v — a hit's (s, t) is their affine combination, on a parallelogram too; t points up
 * (t = 1 is the image's top row).  tex_id: an index into the RtScene.textures the scene was created with, whose DECODED width x height
 * (RtTexture.width / height, nbytes = 3 width height) is the image; RT_FLAT_IMAGE_NONE: no image, the rest of the entry is ignored.
 * wrap_s, wrap_t: what a coordinate outside [0, 1) does, RT_WRAP_REPEAT (tile) or RT_WRAP_CLAMP (the edge texel).  The fetch is the nearest
 * texel.  csrc/common/rt_flat_image.h holds the contract step by step. */
#define RT_FLAT_IMAGE_NONE 0xFFFFFFFFu
#define RT_WRAP_REPEAT 0u
#define RT_WRAP_CLAMP 1u
typedef struct RtFlatImage {
  double uv[6];
  uint32_t tex_id;
  uint32_t wrap_s, wrap_t;
  uint32_t reserved;  /* must be 0 */
} RtFlatImage;

/* config.rs:66-75 Config, with the camera already derived (camera.rs:45-77). */
typedef struct RtScene {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t width, height;
  uint32_t samples_per_pixel;
  uint32_t max_depth;
  uint32_t sky_mode; /* RT_SKY_* */
  double cam_origin[3];
  double cam_lower_left[3];
  double cam_horizontal[3];
  double cam_vertical[3];
  const uint8_t* sky_rgb8; /* sky_mode==TEXTURE */
  uint64_t sky_w, sky_h;
  const RtSphere* spheres;
  uint32_t n_spheres;
  uint32_t n_textures;
  const RtTexture* textures;
  uint64_t seed; /* Philox key; replaces rand::thread_rng (raytracer.rs:78,192) */
  uint32_t n_gpus;   /* rt_render_rgb8 only: GPUs to shard the frame over by interleaved scanline tiles;
                      * 0 = the RT_GPUS environment variable, else 1.  More than rt_hip_device_count()
                      * is RT_ERR_INVALID.  The frame is bit-identical for every value. */
  uint32_t reserved0;
} RtScene;

/* Which scanline tiles to render.  Tile k covers rows [k*tile_rows, (k+1)*tile_rows).
 * This call renders tiles first_tile, first_tile+tile_stride, ... and packs them back to
 * back in the output (local tile j <-> global tile first_tile + j*tile_stride).
 * NULL, or tile_rows==0, means the whole frame.  Rank r of G GPUs uses {T, r, G}. */
typedef struct RtRowTiles {
  uint32_t tile_rows;
  uint32_t first_tile;
  uint32_t tile_stride;
} RtRowTiles;

typedef struct RtStats {
  uint64_t samples;      /* camera paths traced = pixels * spp                              */
  uint64_t segments;     /* ray_color invocations that ran hit_world (raytracer.rs:83)      */
  uint64_t sphere_tests; /* ALGORITHMIC ray-sphere tests = segments * n_spheres             */
  uint64_t exact_tests;  /* f64 Sphere::hit evaluations actually executed (after culling)   */
  uint64_t tex_oob;      /* texture fetches the reference would have panicked on            */
  double kernel_ms;      /* device time of the render kernel(s)                             */
  double frame_ms;       /* wall time of the whole call                                     */
  uint64_t grid_steps;   /* cells entered by the grid walks of hit_world (0: no grid)       */
  /* wave-level trip counts (diagnostics of SIMT efficiency; 0 from the CPU oracle):
   * [0] iterations of the segment loop, [1] of the cell-step loop, [2] of the exact-test loop,
   * [3] work items.  lane utilisation of hit_world = segments / (64 * wave_iters[0]) */
  uint64_t wave_iters[4];
  /* shader-clock cycles summed over waves per kernel section; only filled by builds with
   * -DRT_PROFILE (tools/ab_bench.py "prof" arm): [0] sample refill, [1] `large` list,
   * [2] lane_shade, [3] grid entry + walk, [4] pixel sums + tile bookkeeping, [5] item fetch, [6] whole wave */
  uint64_t prof_cycles[12]; /* ... [7] longest wave, [8] shortest wave, [10] waves launched */
  /* CPU oracle only (0 from the GPU): segments traced inside the light loop of a hit on a Light sphere,
   * whose sum raytracer.rs:124 throws away (`None => albedo`).  The kernel does not trace them:
   * kernel.segments == oracle.segments - oracle.segments_discarded, exactly. */
  uint64_t segments_discarded;
  uint32_t n_gpus_used; /* rt_render_rgb8: devices the frame was sharded over (1 elsewhere) */
  uint32_t segments_repeated; /* lit scenes whose light records are a pool: segments traced a second time because no record was
                               * free (counted once in `segments`; their exact tests and grid steps are counted as done); saturates */
  double gather_ms; /* rt_hip_group_*: what the frame spent NOT rendering, on device 0's clock: (start of rank 0's kernel -> frame in
                     * scanline order on device 0) minus kernel_ms of the slowest rank = launch skew between the ranks + the gather +
                     * the de-interleave.  (Until ABI v3 it started at the END of rank 0's kernel and so held the load imbalance.) */
  double setup_ms;  /* rt_render_rgb8: HIP context + table build + scene upload, NOT part of frame_ms
                     * (frame_ms is the window the reference times, raytracer.rs:259-263: the parallel loop
                     * until the pixels are in the caller's buffer) */
  /* rt_hip_group_*: host clock, microseconds since the frame's submit was entered (0 elsewhere):
   * [0] the last rank's host thread is running, [1] the last rank's launch (+ its side of the transfer) is enqueued,
   * [2] the submitting thread knows that, [3] the gather is enqueued (ncclGroupEnd returned / the peer copies' events are
   * waited for), [4] submit returns (de-interleave + device-to-host copy enqueued), [5] collect saw the frame assembled on
   * device 0, [6] ... and in the caller's buffer (= frame_ms), [7] the ranks' counters are read: collect returns.
   * A blocking frame's non-kernel time is frame_ms - kernel_ms; [5]/[6] of a pipelined frame include the wait of its collect. */
  double group_us[8];
} RtStats;

/* rows this call renders (its packed RGB8 output is rows*width*3 bytes) */
static inline uint32_t rt_tiles_local_rows(uint32_t height, const RtRowTiles* tiles) {
  if (!tiles || tiles->tile_rows == 0 || tiles->tile_stride == 0) return height;
  uint32_t rows = 0;
  uint64_t n_tiles = ((uint64_t)height + tiles->tile_rows - 1) / tiles->tile_rows;
  for (uint64_t k = tiles->first_tile; k < n_tiles; k += tiles->tile_stride) {
    uint64_t r0 = k * tiles->tile_rows, r1 = r0 + tiles->tile_rows;
    if (r1 > height) r1 = height;
    rows += (uint32_t)(r1 - r0);
  }
  return rows;
}
/* global row of local packed row `lr` (inverse of the packing above) */
static inline uint32_t rt_tiles_global_row(const RtRowTiles* tiles, uint32_t lr) {
  if (!tiles || tiles->tile_rows == 0 || tiles->tile_stride == 0) return lr;
  uint32_t j = lr / tiles->tile_rows, r = lr % tiles->tile_rows;
  return (tiles->first_tile + j * tiles->tile_stride) * tiles->tile_rows + r;
}

/* Where scanline y of the assembled frame sits in a gather buffer of G ranks, each contributing `pad_rows` packed rows
 * (rank r's rows are rt_tiles_global_row({tile_rows, r, G}, 0..)): the inverse of the packing above, used by the
 * de-interleave kernel of rt_hip_group_* and by any host that assembles the ranks' tiles itself. */
static inline uint32_t rt_tiles_stacked_row(uint32_t y, uint32_t n_ranks, uint32_t tile_rows, uint32_t pad_rows) {
  const uint32_t k = y / tile_rows, r = k % n_ranks, j = k / n_ranks;
  return r * pad_rows + j * tile_rows + y % tile_rows;
}

/* ------------------------------------------------------------------------------------
 * librt_host.so — host plumbing (stays on the CPU, like main.rs/config.rs/camera.rs)
 * ---------------------------------------------------------------------------------- */
typedef struct RtSceneFile RtSceneFile; /* owns the RtScene and every buffer it points to */

/* main.rs:14-15: read + parse a scene file; texture paths resolve relative to cwd. */
int rt_scene_load_file(const char* json_path, RtSceneFile** out);
int rt_scene_load_string(const char* json_text, size_t len, RtSceneFile** out);
/* where a load went, milliseconds: out = {reading the file, parsing the JSON text, the longest JPEG decode (the textures are
 * decoded concurrently, beside the parse), the whole call}; the CLI prints them under RT_STATS=1 */
void rt_scene_load_timings(const RtSceneFile*, double out[4]);
const RtScene* rt_scene_get(const RtSceneFile*);
RtScene* rt_scene_get_mut(RtSceneFile*); /* tests override width/height like raytracer.rs:272-273 */
void rt_scene_free(RtSceneFile*);
/* serde_json::to_string(&config) — exact strings of config.rs:101,128 */
int rt_scene_to_json(const RtSceneFile*, char* buf, size_t cap, size_t* needed);
const char* rt_host_last_error(void);

/* camera.rs:45-77 Camera::new: out = origin[3], lower_left[3], horizontal[3], vertical[3], focal_length */
void rt_camera_derive(const double look_from[3], const double look_at[3], const double vup[3],
                      double vfov_deg, double aspect, double out[13]);
/* camera description of a loaded scene file (camera.rs:29-36): look_from[3], look_at[3], vup[3], vfov, aspect */
void rt_scene_camera(const RtSceneFile*, double out[11]);
/* Thin lens (an extension of the schema; the reference ignores both keys): the camera map's optional "aperture"
 * (default 0: the pinhole) and "focus_dist" (default |look_from - look_at|).  out = aperture, focus_dist as resolved. */
void rt_scene_lens(const RtSceneFile*, double out[2]);
/* Motion blur (an extension of the schema; the reference ignores the key): a sphere map's optional "center1", its
 * centre at shutter close ("center" is the centre at shutter open).  n_spheres x 3 values, center1 of each sphere (= its centre for a
 * sphere without the key), or NULL when no sphere of the file has the key.  Owned by the scene file.  The loader rejects a
 * duplicate center1, a non-finite center1 - center and center1 on a Light sphere. */
const double* rt_scene_motion(const RtSceneFile*);
/* Quads and boxes (an extension of the schema; the reference's loader rejects both forms: missing `center`).  An element
 * of "objects" with the keys "q", "u", "v", "material" (points {x, y, z}) instead of "center", "radius" is a quad;
 * {"box": {"min": [x, y, z], "max": [x, y, z]}, "material": ...} is an axis-aligned box (min_c < max_c on every axis) that expands, in
 * place in the quad order, to the six quads csrc/common/rt_quad.h lists, in that order, built with the operations listed there
 * (rt_scene_to_json writes the six quads).  Spheres keep their relative order in RtScene.spheres, quads theirs here.  The quads of
 * the file, *n of them, or NULL (and *n = 0) for a file without one.  Owned by the scene file.  The loader rejects, naming objects[i]
 * by the file's own index: mixed keys, a duplicate key, "center1" on a quad, a degenerate quad, a material a quad cannot have.
 * Triangles and meshes (extensions too).  {"q", "u", "v", "shape": "triangle" | "parallelogram", "material"} is the
 * canonical form of a flat primitive ("shape" absent = parallelogram; rt_scene_to_json writes "shape" for a triangle, so a file
 * without one serialises as it did).  {"triangle": [a, b, c], "material": M} is Q = a, u = b - a, v = c - a (one subtraction per
 * component).  {"mesh": {"vertices": [[x, y, z], ...], "faces": [[i, j, k], ...]}, "material": M} expands in place, in face order, to
 * its triangles (vertices[i], vertices[j], vertices[k]), as a box expands to its quads.  RtQuad.reserved = RT_QUAD_SHAPE_*.  Rejected,
 * naming objects[i]: an unknown shape, a face without exactly three indices, an index out of range or not an integer, a non-finite
 * vertex, a degenerate (collinear) triangle (naming its face), mixed or duplicate keys, "center1"; more than RT_MAX_QUADS entries in
 * total is RT_ERR_UNSUPPORTED. */
const RtQuad* rt_scene_quads(const RtSceneFile*, uint32_t* n);
/* Shading normals (an extension too): "normals" inside a "mesh" (one [x, y, z] per vertex) or beside a "triangle" (three),
 * or "smooth": true inside a "mesh" (per vertex the sum of cross(u_f, v_f) over the faces that use it, in face order).  *n x 9 f64, the
 * normals at q, q + u, q + v of every entry of rt_scene_quads as written — not normalised; nine zeros for an entry without — what
 * rt_hip_scene_set_flat_normals takes.  NULL and 0 when no entry has normals.  Owned by the RtSceneFile.  rt_scene_to_json writes a
 * triangle that has normals as its exact q, u, v with "shape": "triangle" and "normals": load -> write -> load is bit for bit. */
const double* rt_scene_flat_normals(const RtSceneFile*, uint32_t* n);
/* Motion within the frame (an extension too): an optional "move": [dx, dy, dz] (or {"x", "y", "z"}) on the object map of a
 * quad, a "triangle", a "box" or a "mesh" — a box or a mesh gives it to every face.  *n x 3 f64, the displacement over the open shutter
 * of every entry of rt_scene_quads as written, three zeros for an entry without — what rt_hip_scene_set_flat_motion takes.  NULL and 0
 * when no object has the key.  Owned by the RtSceneFile.  A duplicate key or a non-finite value is a load error naming objects[i];
 * rt_scene_to_json writes the key only where the file had it: load -> write -> load is bit for bit. */
const double* rt_scene_flat_motion(const RtSceneFile*, uint32_t* n);
/* Area lights (an extension too): an optional "emit": [r, g, b] (or {"x", "y", "z"}) on the object map of a quad, a
 * "triangle", a "box" or a "mesh" — a box or a mesh gives it to every face.  *n x 3 f32, the emission of every entry of rt_scene_quads as
 * written, three zeros for an entry without — what rt_hip_scene_set_flat_lights takes.  NULL and 0 when no object has the key.  Owned by
 * the RtSceneFile.  A duplicate key, a component that is not finite or outside [0, 1], "emit" on a sphere, or "emit" together with a
 * non-zero "move" is a load error naming objects[i]; rt_scene_to_json writes the key only where the file had it: load -> write -> load is
 * bit for bit. */
const float* rt_scene_flat_emit(const RtSceneFile*, uint32_t* n);
/* Images (an extension too): an optional "image": {"pixels": "path.jpg", "wrap": "repeat" | "clamp" | [ws, wt]} on the
 * object map of a quad, a "triangle", a "box" or a "mesh", with an optional "uvs": beside q/u/v three pairs (s, t) for Q, Q + u, Q + v
 * (default (0,0), (1,0), (0,1)); beside "triangle" three pairs for a, b, c; inside "mesh" one pair per vertex (required with "image"); a
 * box takes the default on each face.  The file is decoded like a Texture material's and shares its table (rt_scene_get()->textures).
 * *n entries in the order of rt_scene_quads — what rt_hip_scene_set_flat_images takes —, tex_id RT_FLAT_IMAGE_NONE for an entry without.
 * NULL and 0 when no object has the key.  Owned by the RtSceneFile.  "image" on a sphere, "uvs" without "image" or on a box, a duplicate
 * key, a non-finite component, an unknown wrap, a uv count other than the vertex count, or a material other than Lambertian or Metal is a
 * load error naming objects[i]; rt_scene_to_json writes the keys only where the file had them: load -> write -> load is bit for bit. */
const RtFlatImage* rt_scene_flat_images(const RtSceneFile*, uint32_t* n);
/* The structure over the flat primitives (an extension too): a top-level "flat_bvh": true beside "camera" and "objects"
 * asks for rt_hip_scene_create_flats_bvh / rt_hip_group_create_flats_bvh and lifts the loader's cap from RT_MAX_QUADS to RT_MAX_FLATS_BVH
 * (the entry that crosses it is still named by its objects[i]).  1 for such a file, 0 when the key is false or absent: today's behaviour.
 * A value that is not a boolean is a load error.  rt_scene_to_json writes the key only when it is true. */
int rt_scene_flat_bvh(const RtSceneFile*);
/* Camera::new with a thin lens of focus distance f, r = aperture / 2: out = origin[3], lower_left[3], horizontal[3], vertical[3]
 * (on the focus plane), focal_length, u[3], v[3], r.  aperture 0: the pinhole — the first 13 values are rt_camera_derive's bits,
 * whatever focus_dist.  What rt_hip_set_camera and rt_hip_set_lens take. */
void rt_camera_derive_lens(const double look_from[3], const double look_at[3], const double vup[3], double vfov_deg, double aspect,
                           double aperture, double focus_dist, double out[20]);
/* raytracer.rs:220-229 find_lights: writes indices of Light spheres in object order */
uint32_t rt_find_lights(const RtSphere* spheres, uint32_t n, uint32_t* out_idx, uint32_t cap);
/* materials.rs:213-219 load_texture_image: Huffman JPEG (baseline, extended sequential, progressive; 8 bit, 1 or 3
 * components) -> RGB8 (malloc'd, free with rt_free) */
int rt_jpeg_decode_file(const char* path, uint8_t** rgb8, uint32_t* w, uint32_t* h);
int rt_jpeg_decode_mem(const uint8_t* data, size_t len, uint8_t** rgb8, uint32_t* w, uint32_t* h);
const char* rt_jpeg_last_error(void); /* why the last rt_jpeg_decode_* of this thread returned RT_ERR_TEXTURE */
/* raytracer.rs:33-42 write_image: PNG, ColorType::RGB(8) */
int rt_png_write_rgb8(const char* path, const uint8_t* rgb8, uint32_t w, uint32_t h);
void rt_free(void*);

/* ------------------------------------------------------------------------------------
 * librt_hip.so — the hot path on gfx950 (replaces raytracer.rs:260-262)
 * ---------------------------------------------------------------------------------- */
typedef struct RtHipScene RtHipScene; /* scene tables + textures resident in HBM on one GPU */

/* Layout check for foreign-language bindings: sizeof of "RtSphere", "RtTexture",
 * "RtScene", "RtRowTiles", "RtStats" as THIS library was compiled, 0 for an unknown name.  A binding
 * compares them with its own struct sizes once at start-up; rt_abi_version() returns RT_ABI_VERSION. */
size_t rt_abi_sizeof(const char* struct_name);
uint32_t rt_abi_version(void);

int rt_hip_device_count(void);
/* Bring the runtime up on `device` ahead of the first scene: its context, its queues, this library's code object — tens of
 * milliseconds that rt_hip_scene_create otherwise pays for the first scene of a process.  Optional and idempotent; the CLI calls it
 * on a thread while it reads the scene file. */
int rt_hip_device_warm(int device);
const char* rt_hip_last_error(void);
/* Where set-up time went: the stages of the most recent rt_hip_group_create / rt_render_rgb8 of this process (rank 0's scene —
 * table build, texel conversion, uploads, kernel configuration — and the group's own work: streams, frame buffers, transport,
 * pinned staging) as one JSON object {"stage": milliseconds, ...}.  Diagnostics (the CLI prints it under RT_STATS=1); the
 * pointer is valid until the calling thread's next call. */
const char* rt_hip_setup_profile(void);
/* Upload scene tables, textures and sky to HBM of `device`.  The caller may free the
 * RtScene and everything it points to as soon as this returns. */
int rt_hip_scene_create(const RtScene* scene, int device, RtHipScene** out);
/* Motion blur: the scene whose sphere i moves linearly from its centre (shutter open) to center1[3i .. 3i+2] (shutter
 * close).  Each sample of a pixel draws its shutter time tau from its own Philox address and traces its whole path at tau; a sphere is
 * at c0 + dv * tau, dv = center1 - center (f64).  The grid lists each moving sphere by its swept box (rt_hip_scene_update_spheres moves the spheres later).
 * center1 NULL, or equal to every centre: the static scene of rt_hip_scene_create.  RT_ERR_INVALID for a non-finite center1 - center
 * or a moving Light sphere.  rt_hip_scene_query "motion" = the number of moving spheres. */
int rt_hip_scene_create_moving(const RtScene* scene, const double* center1, int device, RtHipScene** out);
/* Participating media: a sphere of kind RT_MAT_MEDIUM scatters a ray at a random depth INSIDE the ball instead of on its
 * surface.  The contract, IEEE f64 without contraction, for the segment with RNG node `node`, origin o, direction d and medium sphere i
 * (centre at the sample's shutter time, like any sphere):
 *   a, half_b, disc, sq as Sphere::hit forms them (sphere.rs:47-55); t1 = ((-half_b) - sq) / a, t2 = ((-half_b) + sq) / a;
 *   disc < 0: no candidate.  t_in = t1 > 0.001 ? t1 : 0.001; !(t_in < t2): no candidate.
 *   len = sqrt(a), inside = (t2 - t_in) * len.
 *   W = philox(pixel, sample, node, 0x80000000 | i), u = u01_53(W.x, W.y): ONE draw per (node, sphere) — the candidate is the same
 *   however often and in whatever order the sphere is tested, and overlapping media draw independently (their densities add).
 *   E = rt_neg_log(1.0 - u) (csrc/common/rt_neg_log.h: its bits are part of the contract), dist = E / density;
 *   !(dist <= inside): no candidate.  t = t_in + dist / len.
 * The candidate enters the closest-hit rule like a surface root: t > 0.001, and t < closest, or t == closest and i < best.
 * Scatter: direction = random_in_unit_sphere(node) (slots 1 + attempt, not normalised), or the incoming d if that is near_zero;
 * attenuation = albedo; no normal.  For the light-sampling draw a medium counts as not Glass.  Denoising AOVs of a first hit in a medium:
 * its albedo, normal (0, 0, 0), the usual 1 / t.
 * rt_hip_scene_create* returns RT_ERR_INVALID for a medium whose radius or density is not finite and > 0, and RT_ERR_UNSUPPORTED for a
 * medium in a scene of more than 65 535 spheres (wide tables have no MEDIUM kernels).  rt_hip_scene_query "media" = their number. */
/* Solid textures: spheres of kind RT_MAT_CHECKER and RT_MAT_NOISE scatter as Lambertian does (the same
 * random_in_unit_sphere draw, the same near_zero rule, "not Glass" for the light-sampling draw, negative radii allowed); their
 * attenuation is a function of the hit point in the SPHERE'S frame.  The contract, IEEE f64 without contraction (the code, whose bits
 * are the contract, is csrc/common/rt_solid.h; its header states every step):
 *   q = hit point - the centre the accepted hit test used (for a moving sphere the centre at the sample's shutter time: the pattern
 *   rides the ball); p = q * scale per component.
 *   Checker: f_c = floor(p_c); any !(fabs(f_c) < 2^52): even; else ((int64)f_x + (int64)f_y + (int64)f_z) & 1: 0 even, 1 odd.
 *   Noise: the lattice noise N(p) — 0.0 if any !(fabs(p_c) < 2^31); corner hash (i_x+dx)*0x9E3779B1 ^ (i_y+dy)*0x85EBCA77 ^
 *   (i_z+dz)*0xC2B2AE3D ^ seed through the murmur3 finaliser (>>16, *0x85EBCA6B, >>13, *0xC2B2AE35, >>16), Perlin's 2002 gradient rule on
 *   h & 15, smoothstep weights, blended dx innermost, then dy, then dz — and the factor f in [0, 1] of the sphere's mode:
 *     noise: 0.5 * (1.0 + N(p)) clamped to [0, 1];  turbulence: T = fabs(sum over `octaves` passes of w * N(r), w halving, r doubling),
 *     f = min(T, 1.0);  marble: x = 0.15915494309189535 * (p_z + 10.0 * T), s = x - floor(x), m = 1.0 - fabs(2.0 * s - 1.0),
 *     f = m * m * (3.0 - 2.0 * m), 0.0 for a non-finite x.
 *   attenuation_c = (float)(f * (double)albedo_c).
 * Denoising AOVs of a first hit on a solid: the evaluated colour as albedo, the usual normal and 1 / t.
 * rt_hip_scene_create* returns RT_ERR_INVALID for a scale that is not finite and > 0, octaves outside 1..16, a seed above 2^32 - 1 or a
 * mode above 2, and RT_ERR_UNSUPPORTED for a solid in a scene of more than 65 535 spheres (wide tables have no SOLID kernels).
 * rt_hip_scene_query "solids" = the number of Checker and Noise spheres.  A scene without one selects the kernels it always did. */
/* Quads: the scene of rt_hip_scene_create_moving(scene, center1) plus n_quads flat parallelograms.  n_quads == 0 IS
 * rt_hip_scene_create_moving: the same tables, the same kernels.  The contract, IEEE f64 without contraction (the code, whose bits are
 * the contract, is csrc/common/rt_quad.h; its header states every step):
 *   dot(p, q) = (p0 q0 + p1 q1) + p2 q2; cross as in rt_hip_reproject below.
 *   once per quad, on the host: n = cross(u, v), nn = dot(n, n), len = sqrt(nn), N = n / len, D = dot(N, Q), w = n / nn.
 *   per segment (o, d) with the closest hit so far `closest`: den = dot(N, d); fabs(den) < 1e-8 (or NaN): no hit;
 *   t = (D - dot(N, o)) / den, accepted only if t > 0.001 and t < closest; P = o + d t, p = P - Q, alpha = dot(w, cross(p, v)),
 *   beta = dot(w, cross(u, p)); accepted iff 0 <= alpha <= 1 and 0 <= beta <= 1.
 *   record: point P, front_face = dot(d, N) < 0, normal = front_face ? N : -N, t.
 * Triangles: an entry whose `reserved` is RT_QUAD_SHAPE_TRIANGLE.  Every entry has a limit lim, 2.0 for a parallelogram
 * and 1.0 for a triangle, and a hit is accepted iff 0 <= alpha <= 1, 0 <= beta <= 1 AND alpha + beta <= lim (the sum: one IEEE f64
 * addition).  With alpha, beta in [0, 1] the rounded sum never exceeds 2, so a parallelogram accepts what it accepted; for a triangle
 * alpha <= 1 and beta <= 1 follow from the other three comparisons.  A NaN fails every comparison.  Everything else on this page holds
 * for both shapes: order, ids and ties whatever the shapes; RT_MAX_QUADS counts both.  For Glass, front_face comes from N = cross(u, v)
 * / |cross(u, v)|: a closed glass mesh needs outward (counter-clockwise) winding.  Not watertight: two triangles that share an edge
 * each round their own alpha and beta.  A `reserved` above 1 is RT_ERR_INVALID (`quad k: bad shape`).  rt_hip_scene_query "triangles"
 * = the number of triangle entries; rt_hip_scene_table "quad_lim" = the limits, n_quads x 8 bytes, or 0 bytes without a triangle.
 * Order: quads are tested as if they followed every sphere in object order, quad k before quad k + 1, the comparison strict: on an
 * equal t a sphere beats a quad and an earlier quad a later one (raytracer.rs:52-57 extended).  Ids: quad k is object n_spheres + k —
 * in the surface record of rt_hip_render_surface too (rt_hip_reproject_surface takes such an id as "not displaced").
 * Materials: Lambertian, Metal and Glass scatter unchanged (they see only point, normal, front_face and the incoming direction);
 * Checker and Noise follow the solid contract with centre = Q.  A quad occludes light rays, media candidates and the first-hit rays of
 * the AOVs like any surface; a first hit on a quad reports albedo by the material rule, the record's normal, 1 / t and its RT_MAT_*.
 * RT_ERR_INVALID: a non-finite q, u or v; nn zero, subnormal or not finite; a Texture, Light or Medium quad; solid parameters the
 * solid contract refuses.  RT_ERR_UNSUPPORTED: more than RT_MAX_QUADS quads; quads in a scene of more than 65 535 spheres (wide tables
 * have no QUADS kernels).  rt_hip_scene_query "quads" = their number.  rt_hip_scene_update_spheres keeps them where they are; rt_hip_scene_update_flats moves them.  The QUADS kernels
 * read the scene's tables from L2 and use the general colour map, whatever the scene's size and albedos. */
int rt_hip_scene_create_quads(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, int device, RtHipScene** out);
/* rt_hip_scene_create_quads with a structure over the flat primitives: a binary BVH, built on the host, that every QUADS
 * kernel, the AOVs and the surface record walk instead of scanning the list.  THE FRAME IS THE FULL SCAN'S IN EVERY BIT.  Contract: for a
 * segment (o, d) and the (closest_in, best_in) the spheres left, let A be the entries k that the test above accepts against closest_in;
 * the scan returns the entry of A with the smallest (t_k, k) in lexicographic order, or its input unchanged when A is empty.  t_k does not
 * depend on `closest`, so the structure returns exactly this in any visiting order: a sphere still beats a flat primitive on an equal t,
 * an earlier entry a later one, a NaN fails every comparison.  The boxes are padded so that a node is skipped only when no entry below it
 * can be accepted; entries and rays outside the preconditions of that padding (extreme skew, needles, coordinates beyond 2^40; a
 * non-finite ray, |o_k| > 2^40, |d_k| > 2^100) are tested by every ray / take the full scan.
 * Arguments and refusals are rt_hip_scene_create_quads's, but: the cap is RT_MAX_FLATS_BVH (RT_ERR_UNSUPPORTED beyond it); the count is
 * checked before any record is read; n_quads = 0 is RT_ERR_INVALID.  Quads with wide tables stay RT_ERR_UNSUPPORTED.  "variant" 1 runs
 * the full scan over such a scene, whatever its size.  rt_hip_scene_query "flat_bvh" = the node count (0: no structure);
 * rt_hip_scene_table "flat_bvh" = the nodes (64 B each: f64 lo[3], hi[3]; u32 skip, first, count, pad) in depth-first order and
 * "flat_bvh_order" = the u32 order table the leaves index (both 0 bytes without the structure).  rt_hip_scene_update_spheres keeps it;
 * rt_hip_scene_update_flats refits it or builds it anew. */
int rt_hip_scene_create_flats_bvh(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, int device, RtHipScene** out);
void rt_hip_scene_destroy(RtHipScene*);
/* Launch the megakernel for the given row tiles on `stream` (a hipStream_t, NULL = default).
 *   d_rgb8    device buffer, rt_tiles_local_rows()*width*3 bytes, packed, top row first;
 *             4-byte aligned (any hipMalloc'd buffer is)
 *   d_linear  optional device buffer of 3 floats per pixel: mean radiance before the
 *             sqrt gamma (raytracer.rs:207-212) — what the parity tests compare
 * Asynchronous: returns after enqueueing.  Inputs are already in HBM.
 * Limits (all return RT_ERR_* instead of misbehaving):
 *   - NOT re-entrant per scene: an RtHipScene owns ONE tile-queue cursor, counter block and event pair.
 *     Launches of one scene must be ordered on ONE stream at a time (back-to-back launches on the same
 *     stream are fine; rt_hip_wait then reports the last one).  Launching on a second stream while the
 *     first stream still holds unfinished work of this scene is RT_ERR_INVALID (finished = rt_hip_wait()
 *     returned, or the caller drained that stream itself: hipStreamQuery says so).  Use one RtHipScene per concurrent stream
 *     (tables are ~100 KB + textures); distinct scenes and distinct devices are fully independent.
 *   - frames wider than 524 280 pixels or with more than 2^31 pixel tiles are RT_ERR_UNSUPPORTED.
 *   - any sphere count is accepted (the reference scans a Vec<Sphere>, raytracer.rs:52-57); above 65 535 spheres the uniform
 *     grid is built with 32-bit item lists ("wide" tables, rt_hip_scene_query "grid_wide") and stays in L2. */
int rt_hip_render(RtHipScene*, const RtRowTiles* tiles, void* d_rgb8, void* d_linear, void* stream);
/* Block until the last rt_hip_render on this scene finished; fill counters and the HIP-event
 * duration of its kernel (events are recorded on the stream the kernel was launched on). */
int rt_hip_wait(RtHipScene*, RtStats* stats);
/* Options of a resident scene: (key, value) pairs, out-of-range values and unknown keys are RT_ERR_INVALID.  The keys, their
 * ranges and defaults are tabulated in INTEGRATION.md §5 ("samples_per_pixel", "max_depth", "seed" override the scene's
 * values; "variant" 1 = the reference's brute force; the rest shape the work distribution and never the image).
 * rt_hip_group_set_option forwards to every rank's scene and takes "spin_us" itself.
 * "flat_build" (DESIGN.md §26): who builds the structure over the flat primitives when rt_hip_scene_update_flats is called with
 * RT_UPDATE_FLATS_REBUILD.  0 (default): the host, as ever.  1: the device — the order table from one sort per tree depth, the boxes from
 * the refit, the same four tables byte for byte.  Any other value is RT_ERR_INVALID; a scene without the structure accepts the option and
 * nothing changes.  Measured on an MI355X (profiles/flat_device_build_time.json): 2^18 entries 67 ms on the host, 4.6 ms on the device
 * (3.8 ms from a device tensor); 6 405 entries 1.27 ms against 0.90 ms.  The device won at both sizes; smaller scenes were not measured,
 * and there a build is a few launch overheads either way. */
int rt_hip_set_option(RtHipScene*, const char* key, int64_t value);
/* What a resident scene was built into (diagnostics): "n_spheres", "n_lights", "grid_cells" (padded cell table, 8 B each),
 * "grid_items" (u16 each), "grid_wide" (1: more than 65 535 spheres — 16-byte cells, u32 items), "grid_large" (spheres every ray tests), "table_bytes" (geometry + material cores + cell table +
 * item lists: what a workgroup stages into LDS once per launch), "texel_bytes" (textures + sky as 4-byte texels in HBM);
 * of the last launch: "lds_bytes" (dynamic LDS of a workgroup), "lds_tables" (1: the tables were staged in LDS),
 * "light_pool_slots" / "light_base_slots" (lit scenes: records in the workgroup's pools of light frames / colour-map bases),
 * "last_kernel" (the key of the megakernel instantiation that ran, ten bits: quads 512 | solid textures 256 | participating media 128 |
 * moving spheres 64 | thin lens 32 | accumulating 16 | wide tables 8 | lights 4 | every albedo in [0, 1] 2 | tables in LDS 1; wide tables
 * never go with tables in LDS, media, solid textures or quads, and quads never with tables in LDS or the short colour map (bits 1 and
 * 2); -1 before the scene's first launch), "lens" (1:
 * rt_hip_set_lens set a lens, 0: the pinhole), "motion" (spheres that move, rt_hip_scene_create_moving; 0: a static scene), "media"
 * (spheres of kind RT_MAT_MEDIUM), "solids" (spheres and quads of kind RT_MAT_CHECKER or RT_MAT_NOISE), "quads" (rt_hip_scene_create_quads; both shapes),
 * "triangles" (the entries of shape RT_QUAD_SHAPE_TRIANGLE among them), "flat_bvh" (nodes of the structure over the flat primitives,
 * rt_hip_scene_create_flats_bvh; 0: none), "flat_refits" (rt_hip_scene_update_flats calls applied by refit since the structure was last built:
 * 0 after creation and after a rebuild), "flat_build" (the option of that name), "flat_device_builds" (rebuilds whose order table the
 * device built, since creation).  -1 for an unknown key. */
int64_t rt_hip_scene_query(const RtHipScene*, const char* key);
/* Diagnostics: a copy of one resident table, as the kernels read it.  name: "grid" (the GridDesc bytes), "cell_word", "cell_items",
 * "large", "geom", "large_geom", "motion" (empty for a static scene), "quads" (RtQuadRec of csrc/common/rt_quad.h, 128 B each: q, u, v, N, w,
 * D; empty for a scene without quads), "quad_lim" (f64 per entry: 2.0 parallelogram, 1.0 triangle; empty for a scene without a
 * triangle), "flat_bvh" and "flat_bvh_order" (rt_hip_scene_create_flats_bvh: the nodes and the order table; empty without the
 * structure).  A blocking device-to-host copy into out (cap bytes); *needed
 * receives the table's size, and out may be NULL to ask for it.  An unknown name, or a buffer that is too small: RT_ERR_INVALID. */
int rt_hip_scene_table(const RtHipScene*, const char* name, void* out, size_t cap, size_t* needed);
/* Move the spheres of a resident scene.  center = n_spheres x 3 (shutter open), center1 = NULL or n_spheres x 3
 * (shutter close), both host pointers.  Radii, materials, textures, sky, camera, lens and options keep their values.  Blocking, like
 * rt_hip_scene_create; waits for the scene's own unfinished launch first.  The grid is rebuilt on the device, and on RT_OK every
 * resident table (rt_hip_scene_table) is byte for byte what rt_hip_scene_create_moving builds for the same RtScene with these centres;
 * the launch configuration and rt_hip_scene_query "table_bytes", "grid_*", "motion" follow.  The learned tile order, the progressive
 * accumulator, the adaptive buffers and the cached denoise AOVs start over, as after rt_hip_set_camera.  Errors are creation's:
 * RT_ERR_INVALID for a non-finite center1 - center or a moving Light, RT_ERR_UNSUPPORTED for a Medium or solid sphere whose new grid
 * needs wide tables — and after any error the scene renders exactly as before the call.  Device buffers grow when the new grid needs
 * it and are otherwise reused.  A scene whose tables a live view shares (a group's ranks) is RT_ERR_INVALID: rt_hip_group_update_spheres. */
int rt_hip_scene_update_spheres(RtHipScene*, const double* center, const double* center1);
/* Move the flat primitives of a resident scene.  quv = n_quads x 9 f64: q, u, v of every entry, in entry order; n_quads
 * must be the scene's.  Shapes, materials, spheres, camera, lens and options keep their values.  Blocking, like
 * rt_hip_scene_update_spheres; waits for the scene's own unfinished launch first.  Scenes of rt_hip_scene_create_quads (the full scan:
 * only the records are made anew) and of rt_hip_scene_create_flats_bvh.  On RT_OK:
 *   - rt_hip_scene_table "quads" is byte for byte what creation builds for these q, u, v (rt_quad_prepare's bits, computed on the device);
 *   - every frame, AOV buffer and surface record is bit for bit that of a scene freshly created with the new geometry, for "variant" 0 and 1;
 *   - "quad_lim" and the material records are untouched.
 * A scene with the structure is REFIT by default: "flat_bvh_order" and every node's skip, first, count and pad stay, a leaf's box becomes
 * the union of its entries' padded boxes and an inner node's the union of its children's (min and max are exact: the union over all
 * entries below it), always-visited leaves keep their infinite boxes; refitting back to the geometry of the last build restores that
 * build's node table byte for byte.  The frame of such a scene is the full scan's in every bit whatever the tree looks like, so a refit
 * scene renders what a rebuilt one renders; what a refit costs is tree quality, never a bit.  The structure is REBUILT — all
 * four flat tables then byte for byte creation's — when flags holds RT_UPDATE_FLATS_REBUILD, or when the set of entries outside the
 * padding's preconditions differs from the resident one (an entry became a needle, crossed 2^40, or stopped being one).  The rebuild
 * runs on the host, or with rt_hip_set_option "flat_build" 1 on the device (nothing but the status crosses back, and
 * "flat_device_builds" counts it); the rebuild that a changed set of such entries forces always runs on the host, whatever the option
 * says — the counts the tree's shape follows from are others then.
 * rt_hip_scene_query "flat_refits" counts the updates applied by refit since the last build (0 after creation or a rebuild): a caller
 * decides with it when to pay for a rebuild.  RT_UPDATE_FLATS_DEVICE: quv is device memory on the scene's device (8-byte aligned): an
 * update by refit or by a device build then crosses no PCIe but the status readback; a rebuild on the host copies the geometry back first.
 * Every error is RT_ERR_INVALID, with creation's wording where creation has one: a null argument; an unknown flag; n_quads different
 * from the scene's; a scene without flat primitives; a non-finite component ("quad k: ..."); a degenerate entry ("quad k: ..."; of all bad
 * entries the lowest k is reported); a scene whose tables a live view shares (rt_hip_group_update_flats).  After any error the scene
 * renders exactly as before the call and its tables are unchanged.  An update drops what rt_hip_scene_update_spheres drops (the learned
 * tile order, the progressive accumulator with its cached AOVs, the adaptive rounds) and the temporal history (as rt_hip_temporal_reset:
 * moved flat primitives are not followed through the temporal filter).  rt_hip_scene_update_spheres afterwards keeps the moved flat
 * primitives, and a flat update keeps moved spheres.  Device buffers are allocated by the first update and reused from then on. */
#define RT_UPDATE_FLATS_REBUILD 1u   /* build the structure anew (on the host; option "flat_build" 1: on the device): tables byte for byte creation's */
#define RT_UPDATE_FLATS_DEVICE  2u   /* quv is device memory on the scene's device */
int rt_hip_scene_update_flats(RtHipScene*, const double* quv, uint32_t n_quads, uint32_t flags);
/* Shading normals on the triangles of a resident scene (the arithmetic is csrc/common/rt_flat_normal.h, bit for bit).
 * normals = n_quads x 9 f64 in entry order: the normals at q, q + u and q + v of every entry, any length (they are normalised once,
 * here); nine zeros: the entry shades flat.  n_quads must be the scene's.  NULL removes them: the scene is then, table for table and bit
 * for bit, one that never had any.  Only shading changes: the hit test, t, ids, ties and front_face (the geometric normal's) are what
 * they were, and a hit whose interpolated normal is degenerate, points through the face or away from the incoming ray takes the
 * geometric normal.  The frames, rt_hip_render_aovs (the normal of the first hit) and the denoisers follow; the surface record of
 * rt_hip_render_surface keeps what it held.  No kernel key changes: rt_hip_scene_query "last_kernel" is what it was.
 * flags: 0, or RT_UPDATE_FLATS_DEVICE (normals is device memory on the scene's device, 8-byte aligned; only the status crosses back).
 * Blocking; waits for the scene's unfinished launch and drops what rt_hip_scene_update_flats drops.  Scenes of
 * rt_hip_scene_create_quads and rt_hip_scene_create_flats_bvh.  rt_hip_scene_update_flats and rt_hip_scene_update_spheres keep the
 * normals as set (the per-hit side test makes stale normals safe; the caller sets new ones after moving geometry).
 * rt_hip_scene_query "flat_normals" = the entries that have normals (0: none); rt_hip_scene_table "flat_normals" = the 72-byte records
 * (unit vectors; empty without normals).  Every error is RT_ERR_INVALID: a null scene; another flag; n_quads different from the scene's;
 * a scene without flat primitives; a vector that is not finite or whose squared length is zero, subnormal or not finite
 * ("quad k: normal ..."), non-zero normals on a parallelogram ("quad k: normal ..."; of all bad entries the lowest k is reported); a
 * scene whose tables a live view shares (rt_hip_group_set_flat_normals).  After any error the scene renders exactly as before. */
int rt_hip_scene_set_flat_normals(RtHipScene*, const double* normals, uint32_t n_quads, uint32_t flags);
/* Flat primitives that move while the shutter is open (the arithmetic is csrc/common/rt_flat_motion.h, bit for bit).
 * move = n_quads x 3 f64 in entry order: the displacement m of every entry over the open shutter.  At the shutter time tau of a sample
 * (DESIGN.md §14's: the same draw, the same value for every segment of the sample) the entry is the same primitive translated by m tau;
 * u, v and the normal do not change.  The pattern of a Checker or Noise entry and the weights of its shading normals ride with it.  An
 * entry of three zeros is tested on exactly the bits it has in a scene without motion.  n_quads must be the scene's.  NULL, or all
 * zeros, removes the motion: the scene is then, table for table and bit for bit, one that never had any.  A scene with a moving entry
 * selects the MOTION kernels (rt_hip_scene_query "last_kernel"), with or without a moving sphere; "motion" keeps counting spheres.
 * The boxes of the structure are swept (the union of the entry's box at both ends of its motion): the call refits them, or builds the
 * structure anew when an end of a motion takes an entry into or out of the always-visited set, exactly as rt_hip_scene_update_flats
 * does, and the frame stays the full scan's in every bit.  rt_hip_scene_update_flats keeps the motion as set and boxes the new geometry
 * with it.  rt_hip_temporal / rt_hip_reproject keep treating a flat primitive as not displaced between frames.
 * flags: 0, or RT_UPDATE_FLATS_DEVICE (move is device memory on the scene's device, 8-byte aligned; only the status crosses back).
 * Blocking; waits for the scene's unfinished launch and drops what rt_hip_scene_update_flats drops.
 * rt_hip_scene_query "flat_motion" = the entries that move (0: none); rt_hip_scene_table "flat_motion" = the 32-byte records
 * {m0, m1, m2, dot(N, m)}, four -0.0 for an entry that does not move (empty without motion).  Every error is RT_ERR_INVALID: a null
 * scene; another flag; n_quads different from the scene's; a scene without flat primitives; a component of m, or a q + m, that is not
 * finite ("quad k: ..."; of all bad entries the lowest k is reported); a scene whose tables a live view shares
 * (rt_hip_group_set_flat_motion).  After any error the scene renders exactly as before. */
int rt_hip_scene_set_flat_motion(RtHipScene*, const double* move, uint32_t n_quads, uint32_t flags);
/* Area lights: the flat primitives of a resident scene that EMIT.  emit: n_quads x 3 f32 in entry order, host memory.  An
 * entry of three zeros does not emit; any other entry is an emitter: it scatters as the reference's Light does (no scattered ray,
 * materials.rs:65-69), its colour is `emit` instead of (1, 1, 1), from both faces; its own material is ignored while it emits and is what
 * the entry is again when emission is removed.  Every component is finite and in [0, 1].  The light list is the Light spheres in object
 * order (rt_find_lights), then the emitters in entry order; n_lights, in the trigger thresholds and the division of raytracer.rs:100,
 * 111-113, is the total.  A Light sphere is aimed at as before, at its centre; an emitter is SAMPLED: each light ray aims at a fresh point
 * of it — one Philox draw at slot 0xFFFFFFFF of the light ray's node, T = (Q + u a) + v b, a triangle folding a + b > 1 back
 * (csrc/common/rt_flat_light.h holds the contract step by step) — so a flat lamp casts a penumbra.  Q, u, v are read from the entry's
 * resident record when aiming: after rt_hip_scene_update_flats the lamp is aimed at where it now is.  A later call replaces the whole
 * table; NULL, or all zeros, removes emission: the scene is then, table for table and bit for bit, one that never had any.  A scene can
 * gain or lose its lit kernels with the call (rt_hip_scene_query "last_kernel"); rt_hip_scene_update_spheres, rt_hip_scene_update_flats,
 * rt_hip_scene_set_flat_normals and the BVH builds keep emission as set.
 * flags: 0, or RT_UPDATE_FLATS_DEVICE (emit is device memory on the scene's device, 4-byte aligned; it is copied back and checked on the host).
 * Blocking; waits for the scene's unfinished launch and drops what rt_hip_scene_update_flats drops.
 * rt_hip_scene_query "flat_lights" = the emitters, "n_lights" = the total; rt_hip_scene_table "flat_lights" = the emitters' entry indices
 * (u32) in light order, empty without.  RT_ERR_UNSUPPORTED: more than RT_MAX_FLAT_LIGHTS emitters (every sampling hit shoots one ray per
 * light; a lamp is a few faces, not a mesh).  RT_ERR_INVALID: a null scene; another flag; n_quads different from the scene's; a scene
 * without flat primitives; a component of emit that is not finite or lies outside [0, 1] ("quad k: ...", the lowest k); an emitter whose
 * displacement (rt_hip_scene_set_flat_motion) is not zero — a Light sphere cannot move either, and rt_hip_scene_set_flat_motion refuses
 * to move an emitter likewise; a scene whose tables a live view shares (rt_hip_group_set_flat_lights).  After any error the scene renders
 * exactly as before. */
#define RT_MAX_FLAT_LIGHTS 32u
int rt_hip_scene_set_flat_lights(RtHipScene*, const float* emit, uint32_t n_quads, uint32_t flags);
/* Images: the flat primitives of a resident scene that show a picture.  images: n_quads entries in entry order.  An entry
 * with an image scatters exactly as its own material does — which must be Lambertian or Metal: its fuzz, its RNG draws, its absorbed /
 * scattered decision — and its attenuation is the nearest texel at the hit's (s, t) instead of `albedo` (csrc/common/rt_flat_image.h holds
 * the contract step by step; no index can leave the texture, RtStats.tex_oob is never touched).  An entry that also emits
 * (rt_hip_scene_set_flat_lights) emits: its own material, image included, is ignored meanwhile.  The first-hit albedo of rt_hip_render_aovs
 * is the texel too.  A later call replaces the whole table; NULL, or all entries RT_FLAT_IMAGE_NONE, removes the images: the scene is then,
 * table for table and bit for bit, one that never had any.  No kernel key changes.  The (s, t) are relative to the entry's own frame: an
 * image rides its entry through rt_hip_scene_update_flats (refit or rebuild) and rt_hip_scene_set_flat_motion, and
 * rt_hip_scene_update_spheres, rt_hip_scene_set_flat_normals and rt_hip_scene_set_flat_lights keep the images as set.
 * flags: 0, or RT_UPDATE_FLATS_DEVICE (images is device memory on the scene's device, 8-byte aligned).  The records are made on the device
 * from either input.  Blocking; waits for the scene's unfinished launch and drops what rt_hip_scene_update_flats drops.
 * rt_hip_scene_query "flat_images" = the entries with an image; rt_hip_scene_table "flat_images" = the resident records, 64 bytes an entry
 * ({u32 texel_off, W, H, wrap_s | wrap_t << 1; f64 uv[6]}, W = 0: no image), empty without.
 * RT_ERR_INVALID: a null scene; another flag; n_quads different from the scene's; a scene without flat primitives; of all bad entries the
 * lowest k, "quad k: ...": a uv component that is not finite, tex_id >= n_textures, a texture with nbytes != 3 width height or a zero
 * side, or one outside the 2^31 texels the scene keeps resident as 4-byte texels, a wrap value above 1, reserved != 0, an own material
 * other than Lambertian or Metal; a scene whose tables a live view shares (rt_hip_group_set_flat_images).  After any error the scene
 * renders exactly as before. */
int rt_hip_scene_set_flat_images(RtHipScene*, const RtFlatImage* images, uint32_t n_quads, uint32_t flags);
/* Animation (the reference's `anim/frame_%03d.png` workflow, README.md:43-57, main.rs:17): move the
 * camera of a resident scene — the four vectors of camera.rs:52-63 — without touching its tables,
 * and render whole frames of it into a host buffer (internal device framebuffer, blocking). */
int rt_hip_set_camera(RtHipScene*, const double origin[3], const double lower_left[3], const double horizontal[3],
                      const double vertical[3]);
int rt_hip_render_to_host(RtHipScene*, uint8_t* out_rgb8, RtStats* stats);
/* Thin-lens camera (RtScene has no lens, so a scene starts as the pinhole): every sample's camera ray leaves a
 * point of the disc of radius lens_radius spanned by the unit vectors u and v, towards the point of the focus plane that
 * rt_hip_set_camera's vectors name (rt_camera_derive_lens gives all of them).  lens_radius 0 selects the pinhole again; a
 * negative or non-finite radius, or a null vector, is RT_ERR_INVALID and changes nothing.  A real change starts the scene's
 * accumulator over, as rt_hip_set_camera does.  Every launch path follows it: rt_hip_render, rt_hip_accumulate(_tiles), the
 * host forms, rt_hip_render_aovs. */
int rt_hip_set_lens(RtHipScene*, const double u[3], const double v[3], double lens_radius);
/* Progressive rendering: a frame's samples in passes, and the image resolved at any point.  Sample s of pixel p traces the same
 * path whatever the frame's sample count, and pixel sums are exact 2^-40 fixed point, so the passes of any split of [0, N) — any
 * sizes, any order — added up and resolved over N give the frame rt_hip_render makes at samples_per_pixel = N, bit for bit
 * (RGB8, linear radiance, NaN pixels).  An ACCUMULATOR is rt_tiles_local_rows()*width*3 u64 words, packed by RtRowTiles exactly
 * like d_rgb8, 8-byte aligned, zeroed by the caller before its first pass: per pixel channel, bits 0-62 hold the fixed-point sum
 * (value * 2^40, rounded), bit 63 is set if any sample of that channel was NaN.  Two accumulators of disjoint sample ranges merge
 * as ((a | b) & F) | ((a & ~F) + (b & ~F)), F = bit 63.  One accumulator holds at most 2^23 - 1 samples per pixel.
 *
 * Render samples [sample_begin, sample_begin + sample_count) of every pixel of `tiles` and ADD their exact fixed-point sums to
 * d_accum (caller-zeroed device buffer, rt_tiles_local_rows()*width*3 u64, 8-byte aligned); asynchronous like rt_hip_render,
 * rt_hip_wait reports it.  The same rules as rt_hip_render (one stream per scene at a time); passes into one accumulator are
 * ordered on one stream.  sample_count 0 or a misaligned accumulator: RT_ERR_INVALID; sample_begin + sample_count above
 * 2^23 - 1: RT_ERR_UNSUPPORTED — and no work is enqueued. */
int rt_hip_accumulate(RtHipScene*, const RtRowTiles* tiles, uint32_t sample_begin, uint32_t sample_count, void* d_accum, void* stream);
/* d_accum holding n_samples samples per pixel -> d_rgb8 / d_linear (either may be NULL), same packing; asynchronous.
 * n_samples 0: RT_ERR_INVALID; above 2^23 - 1: RT_ERR_UNSUPPORTED.  Not reported by rt_hip_wait. */
int rt_hip_resolve(RtHipScene*, const RtRowTiles* tiles, const void* d_accum, uint32_t n_samples, void* d_rgb8, void* d_linear, void* stream);
/* host-buffer form (the CLI; consumers without a HIP allocator): the next sample_count samples of the whole frame into the scene's own
 * accumulator, resolved over everything it holds, RGB8 copied to out_rgb8; blocking.  The accumulator (width*height*24 bytes) is
 * allocated at first use and starts over after rt_hip_set_camera, rt_hip_set_option "max_depth" / "seed" / "accum_reset";
 * rt_hip_scene_query "accum_samples" says how many samples per pixel it holds.  stats: the pass's kernel. */
int rt_hip_refine_to_host(RtHipScene*, uint32_t sample_count, uint8_t* out_rgb8, RtStats* stats);
/* Adaptive sampling: per-tile sample counts, samples spent where the image is still noisy.  The TILES are the
 * accumulating kernels' own pixel tiles for the scene's options and `tiles`: rt_hip_tile_grid writes {tile width, tile height,
 * tiles_x, tiles_y}; tile id = ty * tiles_x + tx over the packed local rows (edge tiles are cut by the frame).  A tile holding
 * n_t samples [0, n_t) resolves, pixel for pixel, to the frame rt_hip_render makes at samples_per_pixel = n_t, bit for bit.
 *
 * rt_hip_accumulate_tiles: rt_hip_accumulate for just the n_list tiles of d_tile_list (device u32 ids, 4-byte aligned), whose words
 * alone change.  Ids must be distinct (two entries of one tile race in the flush); ids at or above the tile count are skipped.
 * n_list 0, a NULL list or n_list above the tile count: RT_ERR_INVALID, and no work is enqueued.  Leaves the scene's learned queue
 * order alone.  rt_hip_wait reports it; its `samples` counts n_list whole tiles.
 *
 * rt_hip_tile_error: the noise estimate of the listed tiles into d_tile_err[id] (f64, one per tile of the grid; only listed ids in
 * the grid are written).  d_now holds samples [0, n_now), d_prev the first n_prev of them (0 < n_prev < n_now, else RT_ERR_INVALID),
 * so A = prev and B = now - prev are disjoint halves.  Per pixel inside the frame none of whose six words has bit 63 set, in IEEE
 * f64, in exactly this order: a_c = P_c / (n_prev * 2^40), b_c = (Q_c - P_c) / ((n_now - n_prev) * 2^40),
 * d = (|a_0 - b_0| + |a_1 - b_1|) + |a_2 - b_2|, s = ((a_0 + b_0) + (a_1 + b_1)) + (a_2 + b_2), e = d / (1e-4 + sqrt(0.5 * s));
 * the tile's error is the max of e, 0.0 if no pixel counts.  Guidance, not contract: for a grey pixel e is about 1.15 x the sum
 * over channels of the two halves' gap in the PNG's sqrt space (full scale 1.0), so an error of 0.0136 is about one 8-bit level
 * per channel.  Asynchronous, not reported by rt_hip_wait.
 *
 * rt_hip_resolve_tiles: rt_hip_resolve with each pixel divided by its tile's count d_tile_spp[id] (device u32, tiles_x*tiles_y
 * entries, each 1 .. 2^23 - 1; other counts give unspecified pixels).
 *
 * rt_hip_render_adaptive_to_host: one whole adaptive frame, blocking.  N = samples_per_pixel, M = min(min_spp, N).  Round 0
 * renders [0, M/2) and [M/2, M) into every tile with an estimate between them; after the round that brought the tiles to n, a tile
 * goes on iff n < N and its error >= threshold, and the next round adds min(n, N - n) samples to every tile that goes on.
 * threshold 0: every tile reaches N (the one-shot frame); M < 2: the one-shot frame, every count N.  Deterministic.  RGB8 to
 * out_rgb8 (width*height*3), counts to out_tile_spp (tiles_y*tiles_x, may be NULL).  A NaN, negative or infinite threshold, or
 * min_spp 0: RT_ERR_INVALID; N above 2^23 - 1: RT_ERR_UNSUPPORTED.  Its own accumulators (2 x width*height*24 bytes) and per-tile
 * arrays are allocated at first use and freed with the scene; the progressive accumulator is untouched.  stats: samples = the sum
 * of pixels x n_t, counters and kernel_ms summed over the rounds' megakernel launches, frame_ms = the whole call.
 * rt_hip_scene_query "adaptive_rounds" and "adaptive_round_tiles_<i>" / "adaptive_round_spp_<i>" / "adaptive_round_kernel_us_<i>"
 * describe the last such frame's rounds (-1 past the last). */
int rt_hip_tile_grid(const RtHipScene*, const RtRowTiles* tiles, uint32_t out[4]);
int rt_hip_accumulate_tiles(RtHipScene*, const RtRowTiles* tiles, const uint32_t* d_tile_list, uint32_t n_list, uint32_t sample_begin,
                            uint32_t sample_count, void* d_accum, void* stream);
int rt_hip_tile_error(RtHipScene*, const RtRowTiles* tiles, const uint32_t* d_tile_list, uint32_t n_list, const void* d_now, uint32_t n_now,
                      const void* d_prev, uint32_t n_prev, double* d_tile_err, void* stream);
int rt_hip_resolve_tiles(RtHipScene*, const RtRowTiles* tiles, const void* d_accum, const uint32_t* d_tile_spp, void* d_rgb8, void* d_linear,
                         void* stream);
int rt_hip_render_adaptive_to_host(RtHipScene*, double threshold, uint32_t min_spp, uint8_t* out_rgb8, uint32_t* out_tile_spp, RtStats* stats);
/* Denoising: feature buffers of the first hit, and an edge-avoiding a-trous filter guided by them.  Whole frames
 * only: `tiles` must be NULL (RT_ERR_UNSUPPORTED otherwise), frames of at most 1 048 560 rows.
 *
 * AOV RECORD: per pixel 8 f32 (32 B), rows x width packed row-major like a whole-frame d_linear, 16-byte aligned:
 *   {albedo.r, albedo.g, albedo.b, inv_depth, normal.x, normal.y, normal.z, coverage}
 * the means over samples [0, n) of what the camera ray of sample s — the ray rt_hip_render traces first for that sample, same Philox
 * address — meets first.  A hit: albedo = the material colour (Lambertian, Metal), (1, 1, 1) (Glass, and Light: it emits (1, 1, 1)),
 * the texel (Texture); normal = the front-facing unit normal of the hit record; inv_depth = 1 / t; it counts towards coverage.  A
 * miss: albedo = the sky colour of the ray; normal, inv_depth 0; coverage the fraction of the n rays that hit.  Each field is
 * summed in f64 in sample order, divided by n, rounded once to f32.
 *
 * rt_hip_render_aovs: the record of every pixel into d_aov (width*height*32 bytes) on `stream`, asynchronous, not reported by
 * rt_hip_wait.  Reads the scene's tables only: no tile queue, learned order, counters or accumulator changes, so every later frame
 * is byte-identical.  n_samples 0 or a misaligned buffer: RT_ERR_INVALID; above 2^23 - 1: RT_ERR_UNSUPPORTED.
 *
 * rt_hip_denoise: L = iterations (0 .. 8) passes of the filter over d_linear (f32 x 3 per pixel, as rt_hip_resolve writes it) guided
 * by d_aov, into d_out_linear (f32 x 3, 4-byte aligned) and / or d_out_rgb8 (3 bytes per pixel, any alignment, the bytes
 * rt_hip_resolve would make of the filtered radiance); either may be NULL.  Iteration i, stride 2^i, B3-spline taps
 * h = (1/16, 1/4, 3/8, 1/4, 1/16) per axis, in IEEE f32 in exactly this order:
 *   k_c = 4^i / (sc * sc), k_n = 1 / (sn * sn), k_a = 1 / (sa * sa), k_z = 1 / (sz * sz), each min(k, FLT_MAX);
 *   a pixel with a NaN channel is copied; otherwise for each tap q = p + 2^i (dx, dy) inside the frame, dy outer, dx inner, -2 .. 2:
 *     dc2 = (dr dr + dg dg) + db db over this iteration's input colour, dn2, da2 alike over normal and albedo, dz2 = dz dz
 *     (differences q - p), x = ((dc2 k_c + dn2 k_n) + da2 k_a) + dz2 k_z,
 *     W = 1 / (1 + x (1 + x (1/2 + x (f32(1/6) + x / 24)))), w = (h(dx) h(dy)) W;
 *     a tap with w > 0 adds w c to the colour sum and w to the weight sum (f32, tap order); a NaN neighbour or x = inf adds nothing;
 *   out = sum / weight sum per channel.  L = 0: the output linear bits are the input's.
 * The scene owns the filter's ping-pong scratch (width*height*32 bytes, allocated at first use, freed with the scene); no caller
 * buffer is written but the outputs, which must not overlap the inputs (RT_ERR_INVALID).  Asynchronous on `stream`.  More than 8
 * iterations: RT_ERR_UNSUPPORTED; a sigma that is not finite and > 0, a NULL or misaligned input: RT_ERR_INVALID; nothing is enqueued.
 *
 * rt_hip_refine_to_host_denoised: rt_hip_refine_to_host — the same pass into the scene's own accumulator, the same reset rules —
 * with the resolved frame denoised (`iterations` passes, the default sigmas below) before it leaves as RGB8.  The AOVs are computed
 * once per accumulator start, over the first min(RT_DENOISE_AOV_SAMPLES, samples_per_pixel) samples.  Any split of [0, N) into passes
 * gives the same final bytes, since the accumulator does. */
#define RT_DENOISE_AOV_SAMPLES 8u
#define RT_DENOISE_ITERATIONS 2u          /* the CLI's --denoise; the defaults below: the best of a sweep at 16 spp */
#define RT_DENOISE_SIGMA_COLOR 0.25f
#define RT_DENOISE_SIGMA_NORMAL 0.1f
#define RT_DENOISE_SIGMA_ALBEDO 0.1f
#define RT_DENOISE_SIGMA_INV_DEPTH 0.01f
int rt_hip_render_aovs(RtHipScene*, const RtRowTiles* tiles, uint32_t n_samples, void* d_aov, void* stream);
int rt_hip_denoise(RtHipScene*, const RtRowTiles* tiles, const void* d_linear, const void* d_aov, uint32_t iterations, float sigma_color,
                   float sigma_normal, float sigma_albedo, float sigma_inv_depth, void* d_out_linear, void* d_out_rgb8, void* stream);
int rt_hip_refine_to_host_denoised(RtHipScene*, uint32_t sample_count, uint32_t iterations, uint8_t* out_rgb8, RtStats* stats);
/* Temporal denoising for animations: each frame's colour is blended with the previous frame's accumulated colour,
 * fetched where the pixel's first-hit surface was on screen one frame ago.  Whole frames only.
 *
 * HISTORY: per pixel 4 f32 (16 B) {r, g, b, n}, rows x width packed row-major, 16-byte aligned: the accumulated linear radiance and
 * the number of frames in it (0: never reuse this pixel).  A CAMERA is 12 doubles: origin[3], lower_left[3], horizontal[3],
 * vertical[3], the vectors of rt_hip_set_camera.
 *
 * rt_hip_reproject: one step.  d_linear (f32 x 3, as rt_hip_resolve writes it) and d_aov (the AOV record above) are this frame's,
 * rendered with the scene's current camera; d_prev_history, d_prev_aov and prev_camera the previous frame's; d_out_history receives
 * the new history.  Per pixel (x, y) of the w x h frame, with dot(p, q) = (p0 q0 + p1 q1) + p2 q2 and
 * cross(p, q) = (p1 q2 - p2 q1, p2 q0 - p0 q2, p0 q1 - p1 q0), every operation one IEEE operation in exactly this order, no
 * contraction (f64 up to the tap positions, f32 from the weights on):
 *   c = the pixel's colour, g its record.  A NaN channel in c: out = c, n = 0, done.
 *   Pixel centre (the camera ray of rt_hip_render with both jitters 0.5): u = (x + 0.5) / (w - 1), v = (h - (y + 0.5)) / (h - 1),
 *     d = ((lower_left + horizontal u) + vertical v) - origin, per component.
 *   Surface point: hit = g.coverage > 0 and g.inv_depth > 0.  A hit: t = (f64)coverage / (f64)inv_depth,
 *     q = (origin + d t) - origin'.  Else (sky): q = d, a point at infinity.   (' marks the previous camera)
 *   Into the previous camera: A = lower_left' - origin', n0 = cross(horizontal', vertical'), n1 = cross(vertical', A),
 *     n2 = cross(A, horizontal'), det = dot(A, n0), a = dot(q, n0) / det, b = dot(q, n1) / det, e = dot(q, n2) / det.
 *     No history unless a > 0 and a, b, e are finite.  fx = (b / a) (w - 1) - 0.5, fy = (h - (e / a) (h - 1)) - 0.5.
 *     No history unless -1 <= fx < w and -1 <= fy < h (otherwise, or for a NaN, every tap lies outside the frame).
 *   Taps: x0 = floor(fx), y0 = floor(fy), wx = (f32)(fx - x0), wy = (f32)(fy - y0); tap (i, j), j = 0, 1 outer, i = 0, 1 inner, is
 *     pixel (x0 + i, y0 + j) with weight W = (i ? wx : 1 - wx) (j ? wy : 1 - wy).
 *   ez = (f32)((f64)coverage / a) for a hit, 0 for sky: the inv_depth the previous frame recorded for this surface.
 *   A tap counts iff it lies inside the frame; its history has n > 0 and no NaN in r, g, b; |normal' - normal|^2 <= tau_n and
 *     |albedo' - albedo|^2 <= tau_a (each (d0 d0 + d1 d1) + d2 d2 of the f32 differences); and dz dz <= (tau_z ez) (tau_z ez) with
 *     dz = inv_depth' - ez.  (A comparison with a NaN fails: the tap does not count.  Sky matches only sky.)
 *   Over the taps that count, in tap order, from 0: s_c = s_c + W H'_c per channel, sw = sw + W, sn = sn + W H'_n.
 *   History iff sw > 0: hist_c = s_c / sw, m = sn / sw + 1, n = m < n_max ? m : n_max, r = 1 / n,
 *     alpha = alpha_min > r ? alpha_min : r, out_c = hist_c + alpha (c_c - hist_c).  No history: out = c, n = 1.
 * Asynchronous on `stream`; reads the scene's size and camera only; writes no caller buffer but the output.  RT_ERR_INVALID, and
 * nothing is enqueued, for: a NULL buffer or camera; d_linear not 4-byte aligned, another buffer not 16-byte aligned; an output that
 * overlaps an input; a threshold that is not finite and >= 0; alpha_min outside [0, 1]; n_max not >= 1 (infinity is allowed).
 *
 * rt_hip_render_frame_temporal_to_host: frame `frame_index` of an animation on one resident scene, blocking.  In this order:
 * samples [b, b + N) of every pixel, N = samples_per_pixel, b = (frame_index mod F) N, F = floor((2^23 - 1) / N) — consecutive frames
 * trace different samples, frame 0 the one-shot frame's — into an accumulator of its own; the resolve to linear f32; the AOVs of
 * the current view over samples [0, min(RT_DENOISE_AOV_SAMPLES, N)); rt_hip_reproject against the history, AOVs and camera the
 * previous call left (none: every pixel starts at n = 1); rt_hip_denoise (`iterations` passes, the default sigmas) over the NEW
 * history's r, g, b into RGB8.  What is kept for the next call is the colour BEFORE the spatial filter, so the filter's bias is never
 * fed back.  The camera (rt_hip_set_camera, rt_hip_set_lens) and the spheres (rt_hip_scene_update_spheres) may change between calls;
 * a moved sphere is handled by the tap test alone, there are no per-object motion vectors.  History, guides and accumulator
 * (width*height*120 bytes: 24 + 2 x 16 + 2 x 32) belong to the scene: allocated at first use, freed with it; the progressive accumulator is untouched.
 * Frame 0 of a scene without history is rt_hip_refine_to_host_denoised(N, iterations) of a fresh scene, byte for byte.
 * More than 8 iterations or N above 2^23 - 1: RT_ERR_UNSUPPORTED.  stats: the frame's megakernel pass.
 * rt_hip_temporal_configure: alpha_min, n_max and the thresholds the host form passes to rt_hip_reproject (checked as there; the
 * history stays).  A scene starts with the RT_TEMPORAL_* values below: the best point of a 360-point sweep over a 3-degree-per-frame orbit of
 * two scenes full of mirrors and glass, which is why alpha_min is so high (profiles/temporal_bench.json).
 * rt_hip_temporal_reset: drop the history and free its buffers; the next frame starts over.
 * rt_hip_temporal_history: the history the last frame left (width*height*4 f32) into a host buffer, blocking; RT_ERR_INVALID if
 * the scene holds none. */
#define RT_TEMPORAL_ALPHA_MIN 0.5f
#define RT_TEMPORAL_N_MAX 8.0f
#define RT_TEMPORAL_TAU_NORMAL 0.02f
#define RT_TEMPORAL_TAU_ALBEDO 0.3f
#define RT_TEMPORAL_TAU_INV_DEPTH 0.02f
int rt_hip_reproject(RtHipScene*, const void* d_linear, const void* d_aov, const void* d_prev_history, const void* d_prev_aov,
                     const double prev_camera[12], float alpha_min, float n_max, float tau_n, float tau_a, float tau_z, void* d_out_history,
                     void* stream);
int rt_hip_render_frame_temporal_to_host(RtHipScene*, uint32_t frame_index, uint32_t iterations, uint8_t* out_rgb8, RtStats* stats);
int rt_hip_temporal_configure(RtHipScene*, float alpha_min, float n_max, float tau_n, float tau_a, float tau_z);
int rt_hip_temporal_reset(RtHipScene*);
int rt_hip_temporal_history(RtHipScene*, float* out_history);
/* Temporal denoising with surface tracking: the step above told WHICH sphere a pixel shows, what it is made of and
 * where that sphere stood one frame ago — so a moved sphere keeps the history of its own surface, and a mirror or a lens, whose
 * picture first-hit reprojection cannot follow, is given a short history of its own.  Whole frames only.  Opt-in: nothing above changes.
 *
 * SURFACE RECORD: per pixel 16 B {u32 id, u32 kind, f64 t}, rows x width packed row-major, 16-byte aligned.  It describes ONE ray, the
 * pixel-centre ray of the pinhole: u = (x + 0.5) / (w - 1), v = (h - (y + 0.5)) / (h - 1), d = ((lower_left + horizontal u) +
 * vertical v) - origin per component, IEEE f64 with real divisions, from the camera origin even when a lens is set.  Its closest hit by
 * the rule of hit_world (t > 0.001; of equal roots the sphere earlier in the scene wins): id = the sphere's index in the scene's
 * order, kind = its RT_MAT_*, t = the accepted root.  A miss: id = kind = 0xFFFFFFFF, t = 0.0.  A scene with motion
 * (rt_hip_scene_create_moving, rt_hip_scene_update_spheres) has every sphere at shutter time 0.5: centre_k + (center1_k - centre_k) * 0.5
 * in f64.  A scene with media takes the medium candidate of DESIGN.md §15 with the RNG address (this pixel, sample 0, node 0); a first
 * hit inside a medium reports the medium sphere's id and RT_MAT_MEDIUM.
 *
 * rt_hip_render_surface: the record of every pixel into d_surface (width*height*16 bytes) on `stream`, asynchronous, not reported by
 * rt_hip_wait.  Reads the scene's tables and camera only: no tile queue, learned order, counters or accumulator changes, so every later
 * frame is byte-identical.  Every scene rt_hip_render_aovs accepts.  A NULL or misaligned buffer: RT_ERR_INVALID; tiles:
 * RT_ERR_UNSUPPORTED; nothing is enqueued.
 *
 * rt_hip_reproject_surface: one step.  As rt_hip_reproject, with this frame's and the previous frame's surface records
 * (d_surface, d_prev_surface) and d_displacement: NULL (nothing moved), or a device table of n_spheres x 3 f64, sphere i's centre now
 * minus its centre one frame ago, 8-byte aligned.  Per pixel (x, y), every operation one IEEE operation in exactly this order, no
 * contraction (f64 for the geometry and the depth test, f32 from the weights on); dot and cross as above:
 *   c = the pixel's colour, g its AOV record, s its surface record.  A NaN channel in c: out = c, n = 0, done.
 *   Pixel centre: u, v and d as above.
 *   Surface point: hit = s.id != 0xFFFFFFFF.  A hit: q = ((origin + d s.t) - D) - origin' per component, D = d_displacement[s.id];
 *     with a NULL table (or s.id >= n_spheres) there is no subtraction, q = (origin + d s.t) - origin', the bits of D = 0.
 *     Else (sky): q = d.
 *   Into the previous camera: A, n0, n1, n2, det, a, b, e, the two "no history unless" rules, fx and fy exactly as in rt_hip_reproject.
 *   Taps: x0, y0, wx, wy, the tap order and the weights W exactly as in rt_hip_reproject.
 *   A tap counts iff it lies inside the frame; its history has n > 0 and no NaN in r, g, b; its previous surface record has
 *     id' == s.id (sky matches only sky); |normal' - normal|^2 <= tau_n and |albedo' - albedo|^2 <= tau_a as in rt_hip_reproject;
 *     and, for a hit, dt dt <= (tau_z a) (tau_z a) in f64 with dt = t' - a, t' the tap's previous t and tau_z widened to f64
 *     (a is the previous camera's ray parameter of the surface point).  Sky has no depth test.  A comparison with a NaN fails.
 *   Sums, hist_c, m, n and r = 1 / n as in rt_hip_reproject.  floor = alpha_specular if s.kind is RT_MAT_METAL or RT_MAT_GLASS, else
 *     alpha_min; alpha = floor > r ? floor : r, out_c = hist_c + alpha (c_c - hist_c).  No history: out = c, n = 1.
 *   (alpha_specular = 1: such a pixel keeps this frame's colour alone and goes on to the spatial filter.)
 * Asynchronous on `stream`; writes no caller buffer but the output.  RT_ERR_INVALID, and nothing is enqueued, for: a NULL buffer or
 * camera (d_displacement may be NULL); d_linear not 4-byte aligned, d_displacement not 8-byte, another buffer not 16-byte aligned; an
 * output that overlaps an input, the two surface buffers and the displacement table included; a threshold that is not finite and
 * >= 0; alpha_min or alpha_specular outside [0, 1]; n_max not >= 1.
 *
 * rt_hip_temporal_surface: switches rt_hip_render_frame_temporal_to_host between the path above (enable 0, how a scene starts: its
 * bytes are unchanged) and surface tracking; a real change of mode drops the history as rt_hip_temporal_reset does.  alpha_specular
 * (in [0, 1], else RT_ERR_INVALID) is kept either way; rt_hip_temporal_configure supplies the other five values in both modes
 * (RT_TEMPORAL_SURFACE_* below are what the CLI's --temporal-surface configures: the best point of a sweep over alpha_min, alpha_specular and
 * n_max on four animations, which left n_max and the thresholds at RT_TEMPORAL_*; profiles/temporal_surface_bench.json).  In surface mode a frame is, in this order: the
 * accumulate, the resolve and the AOVs as above; rt_hip_render_surface; rt_hip_reproject_surface against the previous frame's history,
 * AOVs, surface record and camera; rt_hip_denoise over the new history.  The displacement is the scene's own: per temporal frame it
 * keeps each sphere's centre at shutter time 0.5 of the tables that frame rendered with, centre_k + (center1_k - centre_k) * 0.5 in f64,
 * and uploads now - previous before the step (zeros for the first frame), so rt_hip_scene_update_spheres between calls is followed with no
 * extra caller work.  Frame 0 of a scene without history stays rt_hip_refine_to_host_denoised, byte for byte.  The extra buffers
 * (width*height*32 bytes + n_spheres*24) belong to the scene: allocated at first use in surface mode only, freed by
 * rt_hip_temporal_reset and with the scene.  rt_hip_scene_query "temporal_surface": 0 / 1.
 * Not handled: the group (multi-GPU) calls, row tiles, a thin lens (the centre ray is the pinhole's), what a mirror or a lens SHOWS
 * (only its own surface is followed), moving Light spheres (no scene can hold one). */
#define RT_TEMPORAL_SURFACE_ALPHA_MIN 0.5f
#define RT_TEMPORAL_SURFACE_ALPHA_SPECULAR 1.0f
int rt_hip_render_surface(RtHipScene*, const RtRowTiles* tiles, void* d_surface, void* stream);
int rt_hip_reproject_surface(RtHipScene*, const void* d_linear, const void* d_aov, const void* d_surface, const void* d_prev_history,
                             const void* d_prev_aov, const void* d_prev_surface, const double prev_camera[12], const double* d_displacement,
                             float alpha_min, float alpha_specular, float n_max, float tau_n, float tau_a, float tau_z, void* d_out_history,
                             void* stream);
int rt_hip_temporal_surface(RtHipScene*, int enable, float alpha_specular);
/* A frame over the GPUs of one node, scene resident (the parallel loop of raytracer.rs:254-262 spread over devices;
 * animation: README.md:43-57).  n_gpus = 0 takes scene->n_gpus, then RT_GPUS, then 1.  Each rank renders
 * interleaved 2-scanline tiles (RtRowTiles{2, r, G}) on its own host thread and stream; ONE gather per frame
 * (RCCL `ncclGather` over xGMI, or peer copies with RT_GATHER=peer) brings the packed tiles to device 0,
 * a kernel puts the scanlines in order, ONE device-to-host copy delivers them.  Bit-identical for every G.
 * stats: counters summed over ranks, kernel_ms = slowest rank, frame_ms = the whole call, gather_ms. */
typedef struct RtHipGroup RtHipGroup;
/* What a group actually runs on (rt_hip_group_info): bench.py echoes it next to its numbers. */
#define RT_GROUP_INFO_MAX_RANKS 64u
enum { RT_GATHER_NONE = 0, RT_GATHER_RCCL = 1, RT_GATHER_PEER = 2 };
typedef struct RtGroupInfo {
  uint32_t n_ranks;    /* G */
  uint32_t n_devices;  /* distinct HIP device ordinals among the ranks (== n_ranks unless RT_GPUS_EMULATE=1) */
  uint32_t transport;  /* RT_GATHER_*: how the packed tiles reach the first device (NONE: one rank, nothing to gather) */
  uint32_t rccl_comms; /* RCCL communicators created by ncclCommInitAll (n_ranks with RT_GATHER_RCCL, else 0) */
  uint32_t tile_rows;  /* scanlines per interleaved tile (2) */
  uint32_t pad_rows;   /* rows of one rank's slice of the gather buffer */
  uint32_t emulated;   /* 1: ranks share devices (RT_GPUS_EMULATE=1, tests) */
  uint32_t transport_fallback; /* 1: RCCL was wanted but could not be used (library, communicators or its self-test gather failed):
                                * the group runs on peer copies instead; rt_hip_group_fallback_reason() says why */
  int32_t device[RT_GROUP_INFO_MAX_RANKS]; /* device ordinal of rank r; -1 beyond n_ranks */
} RtGroupInfo;
/* One rank of a group (rt_hip_group_ranks): where it runs and what its last frame cost — enough for one bench line of an
 * N-GPU run to explain its own efficiency. */
typedef struct RtGroupRank {
  int32_t device;        /* HIP device ordinal */
  int32_t numa_node;     /* NUMA node of the device's PCI function (sysfs numa_node), -1 unknown */
  int32_t pinned_cpus;   /* CPUs in the affinity mask the rank's host thread was pinned to (that node's), 0: not pinned */
  int32_t peer_to_root;  /* hipDeviceCanAccessPeer(this device -> the first rank's device); 1 for rank 0 and shared devices */
  char pci_bus_id[16];   /* "0000:c1:00.0" */
  double kernel_ms;      /* the frame collected last: this rank's kernel (HIP events on its stream) */
  double t_wake_us;      /* the frame submitted last, host clock since its submit was entered: the rank's host thread is running, */
  double t_enq_us;       /* ... its launch (+ its side of the transfer) is enqueued */
} RtGroupRank;
/* Creation never fails because of the TRANSPORT: if RCCL is wanted (the default with one device per rank) but its library
 * cannot be loaded (RT_RCCL_LIB overrides the path), ncclCommInitAll fails, or the self-test gather run at creation fails,
 * times out (RT_RCCL_TIMEOUT_MS, default 20 000) or delivers wrong bytes, the communicators are torn down and the group
 * runs on peer copies (RtGroupInfo.transport = RT_GATHER_PEER, .transport_fallback = 1); a gather that fails to enqueue in a
 * later frame switches the same way and re-sends that frame's tiles.  Rank threads are pinned to the CPUs of their device's
 * NUMA node unless RT_GROUP_PIN=0. */
int rt_hip_group_create(const RtScene* scene, uint32_t n_gpus, RtHipGroup** out);
/* rt_hip_group_create whose every rank is rt_hip_scene_create_moving(scene, center1): motion blur */
int rt_hip_group_create_moving(const RtScene* scene, const double* center1, uint32_t n_gpus, RtHipGroup** out);
/* rt_hip_group_create_moving whose every rank is rt_hip_scene_create_quads(scene, center1, quads, n_quads): quads */
int rt_hip_group_create_quads(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t n_gpus, RtHipGroup** out);
/* rt_hip_group_create_quads whose every rank is rt_hip_scene_create_flats_bvh(scene, center1, quads, n_quads), with its refusals */
int rt_hip_group_create_flats_bvh(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, uint32_t n_gpus, RtHipGroup** out);
int rt_hip_group_info(const RtHipGroup*, RtGroupInfo* info);
uint32_t rt_hip_group_ranks(const RtHipGroup*, RtGroupRank* out, uint32_t cap); /* fills min(cap, n_ranks) entries, returns n_ranks */
const char* rt_hip_group_fallback_reason(const RtHipGroup*);                    /* "" unless RtGroupInfo.transport_fallback */
/* the same frame, left in HBM: scanline order, RGB8, on the group's first device (rt_hip_group_frame returns the device
 * pointer, valid until the group is destroyed, and that device's ordinal) — no device-to-host copy.  Blocking. */
int rt_hip_group_render(RtHipGroup*, RtStats* stats);
const void* rt_hip_group_frame(const RtHipGroup*, int* device_out);
/* The same frame in two halves, for callers that render frame after frame (an animation): submit enqueues everything
 * frame i needs — G launches, the gather, the de-interleave and, if out_rgb8 is not NULL, the copy into that host buffer —
 * and returns; collect blocks until the OLDEST submitted frame is complete and fills its stats.  Two frames may be in flight
 * (a third submit is RT_ERR_INVALID): every buffer exists twice, a rank's tiles travel on a transfer stream of their own,
 * so frame i's gather + copy run while frame i+1 renders and a step costs the slowest rank's kernel.  The camera and
 * options a frame is rendered with are those in force when it is SUBMITTED.  out_rgb8 may be pageable memory: the frame
 * leaves the device into a pinned staging buffer of the group (so submit never blocks on the copy) and collect moves
 * it into out_rgb8, which must stay valid until then; a buffer that is itself pinned (hipHostMalloc / hipHostRegister)
 * is written directly.  rt_hip_group_frame() points at the frame collected last.  rt_hip_group_render / _render_to_host are
 * submit + collect (after collecting whatever was still in flight). */
int rt_hip_group_submit(RtHipGroup*, uint8_t* out_rgb8);
int rt_hip_group_collect(RtHipGroup*, RtStats* stats);
void rt_hip_group_destroy(RtHipGroup*);
uint32_t rt_hip_group_size(const RtHipGroup*);
int rt_hip_group_set_camera(RtHipGroup*, const double origin[3], const double lower_left[3], const double horizontal[3],
                            const double vertical[3]);
int rt_hip_group_set_lens(RtHipGroup*, const double u[3], const double v[3], double lens_radius);  /* rt_hip_set_lens on every rank */
int rt_hip_group_set_option(RtHipGroup*, const char* key, int64_t value);
/* rt_hip_scene_update_spheres on every rank (each rank's tables are built once; its second view follows them).  RT_ERR_INVALID while a
 * submitted frame is uncollected. */
int rt_hip_group_update_spheres(RtHipGroup*, const double* center, const double* center1);
/* rt_hip_scene_update_flats on every rank (each rank's tables are updated once; its second view follows them).  RT_ERR_INVALID while a
 * submitted frame is uncollected, and for RT_UPDATE_FLATS_DEVICE in a group whose ranks are on more than one device. */
int rt_hip_group_update_flats(RtHipGroup*, const double* quv, uint32_t n_quads, uint32_t flags);
/* rt_hip_scene_set_flat_normals on every rank, under the same two conditions. */
int rt_hip_group_set_flat_normals(RtHipGroup*, const double* normals, uint32_t n_quads, uint32_t flags);
/* rt_hip_scene_set_flat_motion on every rank, under the same two conditions. */
int rt_hip_group_set_flat_motion(RtHipGroup*, const double* move, uint32_t n_quads, uint32_t flags);
/* rt_hip_scene_set_flat_lights on every rank, under the same two conditions. */
int rt_hip_group_set_flat_lights(RtHipGroup*, const float* emit, uint32_t n_quads, uint32_t flags);
/* rt_hip_scene_set_flat_images on every rank, under the same two conditions. */
int rt_hip_group_set_flat_images(RtHipGroup*, const RtFlatImage* images, uint32_t n_quads, uint32_t flags);
int rt_hip_group_render_to_host(RtHipGroup*, uint8_t* out_rgb8, RtStats* stats);
/* the group's layout arithmetic as the library compiled it (no GPU needed): rt_tiles_stacked_row() with the group's
 * tile height; *tile_rows_out receives that height (2) */
uint32_t rt_hip_group_stacked_row(uint32_t y, uint32_t n_ranks, uint32_t pad_rows, uint32_t* tile_rows_out);
/* Convenience = the drop-in for render()'s parallel loop (raytracer.rs:254-262): host buffers in,
 * host RGB8 out.  Blocking.  Renders on scene->n_gpus devices (see RtScene.n_gpus / RT_GPUS): the scene
 * is replicated, device r renders scanline tiles r, r+G, ... (2 rows each) on its own host thread and
 * stream, the packed tiles meet on device 0 through ONE gather (RCCL send/recv over xGMI, or peer copies
 * with RT_GATHER=peer), are de-interleaved by a small kernel and leave in ONE device-to-host copy.  The camera is RtScene's: a
 * pinhole (a lens needs a group or scene and rt_hip_set_lens), and every sphere is static (motion blur needs
 * rt_hip_group_create_moving or rt_hip_scene_create_moving).  It takes an RtScene, which holds no quads, so its frames are quad-free
 * (quads need rt_hip_group_create_quads or rt_hip_scene_create_quads). */
int rt_render_rgb8(const RtScene* scene, uint8_t* out_rgb8, RtStats* stats);
const char* rt_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
