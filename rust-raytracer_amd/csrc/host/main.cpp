// main.cpp — `raytracer <config_file> <output_file>`: the reference CLI (main.rs:7-20) with
// the rayon loop of render() (raytracer.rs:250-266) replaced by one rt_render_rgb8() call
// into librt_hip.so.  Same argv, same two stdout lines.  Where the reference panics
// (unreadable / unparsable config, texture or PNG failure) this prints the same message to
// stderr and exits 101, the exit status of a Rust panic.
//
// `Frame time` is the window the reference times (raytracer.rs:259-263: the parallel loop until the pixels are in the
// host buffer) — HIP start-up, table build and scene upload happen before it and are reported under RT_STATS=1.
// RT_GPUS=N (or "n_gpus" in RtScene) shards the frame over N GPUs inside librt_hip.so (rt_hip_group_*).
//
// The modes beyond the reference's (cli_args.h: the flags, and which may stand together) each have a function below, with the mode's
// paragraph above it: progressive(), adaptive(), animate() with its three drivers, one_shot().  What every mode shares about a scene
// file — lens, moving spheres, flat primitives and their structure — is at create(); what every animation driver shares about frame f
// is Anim::pose() and the two apply()s.
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/rt_abi.h"
#include "anim_path.h"
#include "cli_args.h"

namespace {
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
double ms_since(Clock::time_point t) { return ms_between(t, Clock::now()); }

// what a run is made of: the command line and the loaded scene file
struct Run {
  const cli::Options& o;
  RtSceneFile* sf;
  RtScene* sc;  // rt_scene_get_mut(sf)
};

// what the run says when it ends early, and its exit status (usage: main.rs:9-12, a normal return; 101: the exit status of a Rust panic)
int usage(const cli::Options& o) { std::printf("Usage: %s <config_file> <output_file>\n", o.program); return 0; }
int render_failed(int rc) { std::fprintf(stderr, "render failed: %s: %s\n", rt_strerror(rc), rt_hip_last_error()); return 101; }
int write_failed(const char* why) { std::fprintf(stderr, "error writing image: %s\n", why); return 101; }
// how many GPUs the run asks for: RtScene::n_gpus, else RT_GPUS, else 1 (sc null: before the scene is loaded)
long gpus_asked(const RtScene* sc) {
  if (sc && sc->n_gpus) return sc->n_gpus;
  const char* e = std::getenv("RT_GPUS");
  return e ? std::strtol(e, nullptr, 10) : 1;
}

// The resident scene / group of a scene file.  What a scene file may hold beyond the reference's, in every mode:
// Motion blur: a scene whose spheres have "center1" (rt_scene_motion) is created with rt_hip_scene_create_moving /
// rt_hip_group_create_moving, with or without a lens.
// Quads and boxes: a scene file that holds a quad or a box (rt_scene_quads) is created with rt_hip_scene_create_quads /
// rt_hip_group_create_quads.  A quad-free file takes the calls it always took.
// The structure over the flat primitives: a file with "flat_bvh": true (rt_scene_flat_bvh) is created with
// rt_hip_scene_create_flats_bvh / rt_hip_group_create_flats_bvh instead; `--flat-bvh` (with any of the modes, or alone)
// does the same for any file that holds a flat primitive, for A/B runs; on a file without one it changes nothing (there is nothing to build
// over), and given twice it is refused with the usage line.  The frame is the same in every bit.
// Shading normals: a file whose triangles or meshes carry "normals" (rt_scene_flat_normals) has them set right after creation
// (rt_hip_scene_set_flat_normals / rt_hip_group_set_flat_normals); a file without any takes the calls it always took.
int set_normals(RtHipScene* h, const double* n, uint32_t k) { return rt_hip_scene_set_flat_normals(h, n, k, 0u); }
int set_normals(RtHipGroup* h, const double* n, uint32_t k) { return rt_hip_group_set_flat_normals(h, n, k, 0u); }
// Motion within the frame: a file whose quads, triangles, boxes or meshes carry "move" (rt_scene_flat_motion) has it set
// right after creation too (rt_hip_scene_set_flat_motion / rt_hip_group_set_flat_motion) and blurs in every mode a "center1" file blurs in.
int set_motion(RtHipScene* h, const double* m, uint32_t k) { return rt_hip_scene_set_flat_motion(h, m, k, 0u); }
int set_motion(RtHipGroup* h, const double* m, uint32_t k) { return rt_hip_group_set_flat_motion(h, m, k, 0u); }
// Area lights: a file whose quads, triangles, boxes or meshes carry "emit" (rt_scene_flat_emit) has it set right after
// creation too (rt_hip_scene_set_flat_lights / rt_hip_group_set_flat_lights), before the motion: an emitter may not move.
int set_lights(RtHipScene* h, const float* e, uint32_t k) { return rt_hip_scene_set_flat_lights(h, e, k, 0u); }
int set_lights(RtHipGroup* h, const float* e, uint32_t k) { return rt_hip_group_set_flat_lights(h, e, k, 0u); }
// Images: a file whose quads, triangles, boxes or meshes carry "image" (rt_scene_flat_images) has them set right after
// creation too (rt_hip_scene_set_flat_images / rt_hip_group_set_flat_images); they ride their entries through every later update.
int set_images(RtHipScene* h, const RtFlatImage* im, uint32_t k) { return rt_hip_scene_set_flat_images(h, im, k, 0u); }
int set_images(RtHipGroup* h, const RtFlatImage* im, uint32_t k) { return rt_hip_group_set_flat_images(h, im, k, 0u); }
void destroy(RtHipScene* h) { rt_hip_scene_destroy(h); }
void destroy(RtHipGroup* h) { rt_hip_group_destroy(h); }
template <class Handle, class Where>
int create(const Run& r, Where where, Handle** out, int (*moving)(const RtScene*, const double*, Where, Handle**),
           int (*with_quads)(const RtScene*, const double*, const RtQuad*, uint32_t, Where, Handle**),
           int (*with_bvh)(const RtScene*, const double*, const RtQuad*, uint32_t, Where, Handle**)) {
  uint32_t n_quads = 0;
  const RtQuad* quads = rt_scene_quads(r.sf, &n_quads);
  if (!n_quads) return moving(r.sc, rt_scene_motion(r.sf), where, out);
  int rc = (r.o.flat_bvh || rt_scene_flat_bvh(r.sf) ? with_bvh : with_quads)(r.sc, rt_scene_motion(r.sf), quads, n_quads, where, out);
  uint32_t n_normals = 0;
  const double* normals = rt_scene_flat_normals(r.sf, &n_normals);
  if (rc == RT_OK && normals && (rc = set_normals(*out, normals, n_normals)) != RT_OK) { destroy(*out); *out = nullptr; }
  uint32_t n_images = 0;
  const RtFlatImage* images = rt_scene_flat_images(r.sf, &n_images);
  if (rc == RT_OK && images && (rc = set_images(*out, images, n_images)) != RT_OK) { destroy(*out); *out = nullptr; }
  uint32_t n_emit = 0;
  const float* emit = rt_scene_flat_emit(r.sf, &n_emit);
  if (rc == RT_OK && emit && (rc = set_lights(*out, emit, n_emit)) != RT_OK) { destroy(*out); *out = nullptr; }
  uint32_t n_move = 0;
  const double* move = rt_scene_flat_motion(r.sf, &n_move);
  if (rc == RT_OK && move && (rc = set_motion(*out, move, n_move)) != RT_OK) { destroy(*out); *out = nullptr; }
  return rc;
}
int create_scene(const Run& r, int device, RtHipScene** out) {
  return create(r, device, out, rt_hip_scene_create_moving, rt_hip_scene_create_quads, rt_hip_scene_create_flats_bvh);
}
int create_group(const Run& r, RtHipGroup** out) {  // on RT_GPUS devices (default 1)
  return create(r, (uint32_t)0, out, rt_hip_group_create_moving, rt_hip_group_create_quads, rt_hip_group_create_flats_bvh);
}

// Thin lens: a scene whose camera has a non-zero "aperture" renders through the lens in every mode —
// rt_camera_derive_lens gives the camera on the focus plane and the lens, set next to each other on the resident scene or group
// (every --frames camera is re-derived so).
// The scene file's camera with its thin lens, if it has one (aperture != 0): out as rt_camera_derive_lens
bool lens_camera(const RtSceneFile* sf, double out[20]) {
  double cam[11], lens[2];
  rt_scene_camera(sf, cam);
  rt_scene_lens(sf, lens);
  if (lens[0] == 0.0) return false;
  rt_camera_derive_lens(cam, cam + 3, cam + 6, cam[9], cam[10], lens[0], lens[1], out);
  return true;
}
// What progressive() and adaptive() begin with: the scene resident on device 0, through its lens (nothing for a pinhole scene: it keeps
// RtScene's camera), and the first stdout line (main.rs:18).  0, or the exit status.
int open_scene(const Run& r, RtHipScene** hs) {
  double c[20];
  int rc = create_scene(r, 0, hs);
  if (rc == RT_OK && lens_camera(r.sf, c)) {
    rc = rt_hip_set_camera(*hs, c, c + 3, c + 6, c + 9);
    if (rc == RT_OK) rc = rt_hip_set_lens(*hs, c + 13, c + 16, c[19]);
  }
  std::printf("\nRendering %s\n", r.o.output);
  return rc != RT_OK ? render_failed(rc) : 0;
}
std::vector<uint8_t> frame_buffer(const RtScene* sc) { return std::vector<uint8_t>((size_t)sc->width * sc->height * 3); }  // raytracer.rs:254

// Progressive (`raytracer <config_file> <output_file> --passes K`): the scene's samples per pixel in K contiguous ranges, as even
// as they come, each added to the scene's accumulator on the GPU (rt_hip_refine_to_host) and the image so far rewritten to
// <output_file> after every pass (a temporary file in the same directory, then rename: a viewer never sees half a file).  Stderr
// gets `pass i/K: S samples, kernel X ms`; stdout the same two lines as a one-shot run, `Frame time` over all the passes; the
// last PNG is the one-shot run's, byte for byte.  One GPU: RT_GPUS > 1 is refused.
//
// Denoised (`--denoise`, alone or with `--passes K`): every PNG the run writes is the resolved frame passed through the
// feature-guided a-trous filter (rt_hip_refine_to_host_denoised, RT_DENOISE_ITERATIONS iterations, the default sigmas; DESIGN.md
// §12).  The last PNG of `--passes K --denoise` is the `--denoise` run's, byte for byte.  Stdout as a one-shot run.  With --adaptive,
// or with only one of --frames and --orbit: the usage line.  One GPU: RT_GPUS > 1 is refused.  (`--denoise` alone is one pass
// without the pass lines.)
int progressive(const Run& r) {
  const cli::Options& o = r.o;
  const uint32_t passes = o.passes > 0 ? (uint32_t)o.passes : 1u, spp = r.sc->samples_per_pixel;
  RtHipScene* hs = nullptr;
  if (const int status = open_scene(r, &hs)) return status;
  std::vector<uint8_t> pixels = frame_buffer(r.sc);
  const std::string tmp = std::string(o.output) + ".part";  // (same directory: rename() replaces the file in one step)
  double frame_ms = 0.0;
  int status = 0;
  for (uint32_t i = 0; i < passes && status == 0; ++i) {
    const uint32_t count = spp / passes + (i < spp % passes ? 1u : 0u);  // (the first spp % K passes take one sample more)
    RtStats st{};
    int rc = o.denoise ? rt_hip_refine_to_host_denoised(hs, count, RT_DENOISE_ITERATIONS, pixels.data(), &st) : rt_hip_refine_to_host(hs, count, pixels.data(), &st);
    if (rc != RT_OK) { status = render_failed(rc); break; }
    frame_ms += st.frame_ms;
    if (o.passes > 0) std::fprintf(stderr, "pass %u/%u: %u samples, kernel %.3f ms\n", i + 1, passes, count, st.kernel_ms);
    rc = rt_png_write_rgb8(tmp.c_str(), pixels.data(), r.sc->width, r.sc->height);  // raytracer.rs:265
    if (rc == RT_OK && std::rename(tmp.c_str(), o.output) != 0) rc = RT_ERR_PNG;
    if (rc != RT_OK) { status = write_failed(rt_host_last_error()); std::remove(tmp.c_str()); }
    if (i + 1 == passes && status == 0) std::printf("Frame time: %lldms\n", (long long)frame_ms);  // raytracer.rs:263, all the passes
  }
  rt_hip_scene_destroy(hs);
  return status;
}

// Adaptive (`raytracer <config_file> <output_file> --adaptive E [--min-spp M]`, M = 16 by default): one adaptive frame
// (rt_hip_render_adaptive_to_host) — every pixel tile gets samples until its noise estimate falls below E or it
// holds the scene's samples per pixel, and each tile is the one-shot frame at its own count, byte for byte.  Stdout as a one-shot
// run; stderr gets `round i: T tiles at n samples, kernel X ms` per round and what fraction of width x height x spp was traced.
// One GPU: RT_GPUS > 1 is refused.
int adaptive(const Run& r) {
  const RtScene* sc = r.sc;
  RtHipScene* hs = nullptr;
  if (const int status = open_scene(r, &hs)) return status;
  std::vector<uint8_t> pixels = frame_buffer(sc);
  RtStats st{};
  int status = 0;
  const int rc = rt_hip_render_adaptive_to_host(hs, r.o.threshold, (uint32_t)r.o.min_spp, pixels.data(), nullptr, &st);
  if (rc != RT_OK) status = render_failed(rc);
  else {
    std::printf("Frame time: %lldms\n", (long long)st.frame_ms);  // raytracer.rs:263
    const int64_t rounds = rt_hip_scene_query(hs, "adaptive_rounds");
    char key[64];
    for (int64_t i = 0; i < rounds; ++i) {
      int64_t v[3];
      const char* f[3] = {"adaptive_round_tiles_", "adaptive_round_spp_", "adaptive_round_kernel_us_"};
      for (int k = 0; k < 3; ++k) { std::snprintf(key, sizeof key, "%s%lld", f[k], (long long)i); v[k] = rt_hip_scene_query(hs, key); }
      std::fprintf(stderr, "round %lld: %lld tiles at %lld samples, kernel %.3f ms\n", (long long)i, (long long)v[0], (long long)v[1], v[2] / 1000.0);
    }
    const double full = (double)sc->width * sc->height * sc->samples_per_pixel;
    std::fprintf(stderr, "adaptive: %llu samples traced, %.4f of %ux%ux%u, kernel %.3f ms, frame %.3f ms\n", (unsigned long long)st.samples,
                 full > 0 ? st.samples / full : 0.0, sc->width, sc->height, sc->samples_per_pixel, st.kernel_ms, st.frame_ms);
    if (rt_png_write_rgb8(r.o.output, pixels.data(), sc->width, sc->height) != RT_OK) status = write_failed(rt_host_last_error());  // raytracer.rs:265
  }
  rt_hip_scene_destroy(hs);
  return status;
}

// ------------------------------------------------------------------------------------------------------------------ animations
// --flat-frames PREFIX: frame f takes its flat primitives from the scene file PREFIX%03d.json, read with the ordinary loader;
// only its rt_scene_quads are used, and they must be the base file's in count, shapes and materials.  load() returns "" and the
// frame's q, u, v (n x 9), or what is wrong, naming the frame.  (One file at a time: the loader's error text is per process.)
// Shading normals: a frame file has normals on exactly the entries the base file has; they are the frame's (n x 9, empty
// for a scene without any).
struct FlatFrames {
  std::string prefix;
  std::vector<RtQuad> base;
  std::vector<double> base_normals;   // the base file's rt_scene_flat_normals, empty without
  bool moved = false;                 // the base file or some frame file loaded so far has "move" (§27): from then on every frame sets its motion
  bool lit = false;                   // the base file or some frame file loaded so far has "emit" (§28): from then on every frame sets its emission
  std::mutex mu;
  bool on() const { return !prefix.empty(); }
  // move: the frame file's rt_scene_flat_motion (n x 3; all zeros for a file without the key once `moved`), empty while nothing ever moved
  // emit: the frame file's rt_scene_flat_emit (n x 3) likewise
  std::string load(int f, std::vector<double>& out, std::vector<double>& normals, std::vector<double>& move, std::vector<float>& emit) {
    std::lock_guard<std::mutex> lk(mu);
    char path[4096];
    std::snprintf(path, sizeof path, "%s%03d.json", prefix.c_str(), f);
    const std::string which = "frame " + std::to_string(f) + " (" + path + "): ";
    // (§29: the images are the base file's and stay; a frame file brings none — looked for in its text, before the loader would decode a JPEG
    //  per frame: the quoted word is a key of ours alone)
    if (std::FILE* fp = std::fopen(path, "rb")) {
      std::string text;
      char buf[65536];
      for (size_t got; (got = std::fread(buf, 1, sizeof buf, fp)) > 0;) text.append(buf, got);
      std::fclose(fp);
      if (text.find("\"image\"") != std::string::npos) return which + "a frame file takes no `image` (the images are the base file's)";
    }
    RtSceneFile* ff = nullptr;
    if (rt_scene_load_file(path, &ff) != RT_OK) return which + rt_host_last_error();
    uint32_t n = 0;
    const RtQuad* q = rt_scene_quads(ff, &n);
    std::string why;
    if (n != base.size()) why = which + std::to_string(n) + " flat primitives, the scene has " + std::to_string(base.size());
    out.resize(9 * base.size());
    for (uint32_t k = 0; why.empty() && k < n; ++k) {
      if (q[k].reserved != base[k].reserved) why = which + "flat primitive " + std::to_string(k) + " has another shape than the scene's";
      else if (std::memcmp(&q[k].fuzz_or_ior, &base[k].fuzz_or_ior, sizeof(RtQuad) - offsetof(RtQuad, fuzz_or_ior)))
        why = which + "flat primitive " + std::to_string(k) + " has another material than the scene's";
      std::memcpy(&out[9 * (size_t)k], q[k].q, 72);
    }
    uint32_t nn = 0;
    const double* fn = rt_scene_flat_normals(ff, &nn);
    normals.clear();
    if (why.empty() && fn) normals.assign(fn, fn + 9 * (size_t)nn);
    auto has = [](const std::vector<double>& t, size_t k) {
      bool any = false;
      for (int c = 0; c < 9 && !t.empty(); ++c) any = any || t[9 * k + c] != 0.0;
      return any;
    };
    for (size_t k = 0; why.empty() && k < base.size(); ++k)
      if (has(normals, k) != has(base_normals, k)) why = which + "flat primitive " + std::to_string(k) + (has(base_normals, k) ? " has no normals, the scene's has" : " has normals, the scene's has none");
    uint32_t nm = 0;
    const double* fm = rt_scene_flat_motion(ff, &nm);
    move.clear();
    if (why.empty() && fm) { move.assign(fm, fm + 3 * (size_t)nm); moved = true; }
    else if (why.empty() && moved) move.assign(3 * base.size(), 0.0);
    uint32_t ne = 0;
    const float* fe = rt_scene_flat_emit(ff, &ne);
    emit.clear();
    if (why.empty() && fe) { emit.assign(fe, fe + 3 * (size_t)ne); lit = true; }
    else if (why.empty() && lit) emit.assign(3 * base.size(), 0.0f);
    rt_scene_free(ff);
    return why;
  }
};

// Everything about frame f that is host work: what the resident scene or group is told before the frame is rendered.
struct Pose {
  double cam[20];             // rt_camera_derive_lens: origin, lower left, horizontal, vertical (+0, 3, 6, 9), the lens' u, v, radius (+13, 16, 19)
  bool lens = false;          // the scene has a thin lens
  bool spheres = false;       // --shutter: the spheres move to c -> c1 (n x 3 each)
  bool flats = false;         // --flat-frames: the flat primitives move to quv (n x 9)
  uint32_t flat_flags = 0;    // --flat-rebuild K: RT_UPDATE_FLATS_REBUILD on every K-th frame's update
  std::vector<double> c, c1, quv;
  std::vector<double> normals;  // --flat-frames: the frame's shading normals (n x 9), set after its flat primitives; empty: the scene has none
  std::vector<double> move;     // --flat-frames: the frame's motion within the frame (n x 3, §27), set after its flat primitives; empty: nothing ever moved
  std::vector<float> emit;      // --flat-frames: the frame's emission (n x 3, §28), set before its motion; empty: nothing ever emitted
};
// One apply per kind of target.  Each keeps the order of calls its drivers always had (camera first on a scene, last on a group).
// rt_hip_set_camera / rt_hip_group_set_camera refuse null arguments and nothing else, so checking their status changes no run.
int apply(RtHipScene* hs, const Pose& p) {
  int rc = rt_hip_set_camera(hs, p.cam, p.cam + 3, p.cam + 6, p.cam + 9);
  if (rc == RT_OK && p.lens) rc = rt_hip_set_lens(hs, p.cam + 13, p.cam + 16, p.cam[19]);
  if (rc == RT_OK && p.spheres) rc = rt_hip_scene_update_spheres(hs, p.c.data(), p.c1.data());
  if (rc == RT_OK && p.flats) rc = rt_hip_scene_update_flats(hs, p.quv.data(), (uint32_t)(p.quv.size() / 9), p.flat_flags);
  if (rc == RT_OK && p.flats && !p.normals.empty()) rc = rt_hip_scene_set_flat_normals(hs, p.normals.data(), (uint32_t)(p.normals.size() / 9), 0u);
  // (§28: an emitter may not move, whichever call comes second — and the scene still holds the PREVIOUS frame's tables.  A frame that has
  //  both first removes the emission, then sets its motion, then its emission: a frame file is valid in itself, so neither call is refused
  //  for what an earlier frame left behind)
  if (rc == RT_OK && p.flats && !p.emit.empty() && !p.move.empty()) rc = rt_hip_scene_set_flat_lights(hs, nullptr, (uint32_t)(p.emit.size() / 3), 0u);
  if (rc == RT_OK && p.flats && !p.emit.empty() && !p.move.empty()) rc = rt_hip_scene_set_flat_motion(hs, p.move.data(), (uint32_t)(p.move.size() / 3), 0u);
  if (rc == RT_OK && p.flats && !p.emit.empty()) rc = rt_hip_scene_set_flat_lights(hs, p.emit.data(), (uint32_t)(p.emit.size() / 3), 0u);
  if (rc == RT_OK && p.flats && !p.move.empty() && p.emit.empty()) rc = rt_hip_scene_set_flat_motion(hs, p.move.data(), (uint32_t)(p.move.size() / 3), 0u);
  return rc;
}
int apply(RtHipGroup* hs, const Pose& p) {  // (no frame may be in flight while the spheres or the flat primitives move)
  int rc = p.spheres ? rt_hip_group_update_spheres(hs, p.c.data(), p.c1.data()) : RT_OK;
  if (rc == RT_OK && p.flats) rc = rt_hip_group_update_flats(hs, p.quv.data(), (uint32_t)(p.quv.size() / 9), p.flat_flags);
  if (rc == RT_OK && p.flats && !p.normals.empty()) rc = rt_hip_group_set_flat_normals(hs, p.normals.data(), (uint32_t)(p.normals.size() / 9), 0u);
  if (rc == RT_OK && p.flats && !p.emit.empty() && !p.move.empty()) rc = rt_hip_group_set_flat_lights(hs, nullptr, (uint32_t)(p.emit.size() / 3), 0u);   // (as above)
  if (rc == RT_OK && p.flats && !p.emit.empty() && !p.move.empty()) rc = rt_hip_group_set_flat_motion(hs, p.move.data(), (uint32_t)(p.move.size() / 3), 0u);
  if (rc == RT_OK && p.flats && !p.emit.empty()) rc = rt_hip_group_set_flat_lights(hs, p.emit.data(), (uint32_t)(p.emit.size() / 3), 0u);
  if (rc == RT_OK && p.flats && !p.move.empty() && p.emit.empty()) rc = rt_hip_group_set_flat_motion(hs, p.move.data(), (uint32_t)(p.move.size() / 3), 0u);
  if (rc == RT_OK) rc = rt_hip_group_set_camera(hs, p.cam, p.cam + 3, p.cam + 6, p.cam + 9);
  if (rc == RT_OK && p.lens) rc = rt_hip_group_set_lens(hs, p.cam + 13, p.cam + 16, p.cam[19]);
  return rc;
}

// An animation run: what its frames are posed from.
struct Anim {
  const Run& r;
  const int frames;
  const char* const prefix;  // of <prefix>_%03d.png
  double cam[11], lens[2];   // the scene file's (rt_scene_camera, rt_scene_lens)
  FlatFrames flat_files;
  explicit Anim(const Run& run) : r(run), frames(run.o.frames), prefix(run.o.output) {
    rt_scene_camera(r.sf, cam);
    rt_scene_lens(r.sf, lens);
    flat_files.prefix = r.o.flat_frames;
  }
  // camera of frame f: look_from turned about vup around look_at by orbit_deg * f (Rodrigues), then camera.rs:45-77 with the scene's
  // lens = {aperture, focus_dist} (aperture 0: the pinhole, out[0..12] = rt_camera_derive's)
  void orbit_camera(int f, double out[20]) const {
    const double *lf = cam, *la = cam + 3, *up = cam + 6;
    double k[3];
    const double kl = std::sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
    for (int i = 0; i < 3; ++i) k[i] = up[i] / kl;
    const double th = r.o.orbit_deg() * f * (3.14159265358979323846264338327950288 / 180.0), c = std::cos(th), s = std::sin(th);
    const double v[3] = {lf[0] - la[0], lf[1] - la[1], lf[2] - la[2]};
    const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
    const double kx[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
    double from[3];
    for (int i = 0; i < 3; ++i) from[i] = la[i] + v[i] * c + kx[i] * s + k[i] * kv * (1.0 - c);
    rt_camera_derive_lens(from, la, up, cam[9], cam[10], lens[0], lens[1], out);
  }
  // frame f's camera and, with --shutter, its spheres (anim_path.h)
  void view(int f, Pose& p) const {
    orbit_camera(f, p.cam);
    p.lens = lens[0] != 0.0;
    p.spheres = r.o.shutter >= 0.0;
    if (!p.spheres) return;
    p.c.resize(3 * (size_t)r.sc->n_spheres);
    p.c1.resize(p.c.size());
    rt_anim_centres(r.sc->spheres, rt_scene_motion(r.sf), r.sc->n_spheres, f, frames, r.o.shutter, p.c.data(), p.c1.data());
  }
  // with --flat-frames, frame f's flat primitives from its file: "", or what is wrong with the file
  std::string flats(int f, Pose& p) {
    p.flats = flat_files.on();
    p.flat_flags = (r.o.flat_rebuild > 0 && f > 0 && f % r.o.flat_rebuild == 0) ? RT_UPDATE_FLATS_REBUILD : 0u;
    return p.flats ? flat_files.load(f, p.quv, p.normals, p.move, p.emit) : std::string();
  }
  std::string pose(int f, Pose& p) { view(f, p); return flats(f, p); }
  std::string frame_name(int f) const {
    char name[4096];
    std::snprintf(name, sizeof name, "%s_%03d.png", prefix, f);  // main.rs:17
    return name;
  }
};

// What an animation run reports under RT_STATS=1 (one JSON line on stderr): frames per second disk to disk, and per frame the
// kernel (slowest rank), the frame as the reference times it, and its PNG — which of the two bounds the run is then on the line.
struct AnimStats {
  std::mutex mu;
  std::vector<double> kernel_ms, frame_ms, png_ms;
  double host_us[4] = {0, 0, 0, 0};   // the submitting thread's time, summed over the frames: waiting for a free buffer, camera + submit, collect, stdout + hand-over
  explicit AnimStats(int n) : kernel_ms(n, 0.0), frame_ms(n, 0.0), png_ms(n, 0.0) {}
  // a rendered frame's two stdout lines, and its times (distinct elements per frame)
  void frame(const Anim& a, int f, const RtStats& st) {
    std::printf("\nRendering %s\nFrame time: %lldms\n", a.frame_name(f).c_str(), (long long)st.frame_ms);
    kernel_ms[f] = st.kernel_ms; frame_ms[f] = st.frame_ms;
  }
  void report(const char* mode, int frames, unsigned gpus, unsigned writers, double wall_s, double setup_ms) {
    if (!std::getenv("RT_STATS")) return;
    std::string s;
    char buf[256];
    std::snprintf(buf, sizeof buf, "{\"animation\":\"%s\",\"frames\":%d,\"n_gpus\":%u,\"png_writers\":%u,\"setup_ms\":%.3f,\"wall_s\":%.4f,\"frames_per_s\":%.3f", mode, frames, gpus,
                  writers, setup_ms, wall_s, frames / wall_s);
    s = buf;
    auto arr = [&](const char* key, const std::vector<double>& v) {
      s += std::string(",\"") + key + "\":[";
      for (int i = 0; i < frames && i < (int)v.size(); ++i) { std::snprintf(buf, sizeof buf, "%s%.3f", i ? "," : "", v[i]); s += buf; }
      s += "]";
    };
    arr("kernel_ms", kernel_ms); arr("frame_ms", frame_ms); arr("png_ms", png_ms);
    std::snprintf(buf, sizeof buf, ",\"host_us_per_frame\":{\"wait_for_buffer\":%.1f,\"camera_and_submit\":%.1f,\"collect\":%.1f,\"stdout_and_hand_over\":%.1f}",
                  host_us[0] / frames, host_us[1] / frames, host_us[2] / frames, host_us[3] / frames);
    s += buf;
    s += "}\n";
    std::fputs(s.c_str(), stderr);
  }
};

// PNG writers of an animation: W threads take finished frames off a queue; a frame's host buffer (n_buffers of them, owned here)
// goes back to the free list when its file is on disk.  A frame's PNG is itself deflated in parallel bands (scene.cpp), so one
// writer keeps up with the headline frame; the second one is for frames whose kernel is shorter than their PNG (the
// reference's 1 ms test scene).
struct PngWriters {
  struct Job { int frame; uint8_t* px; };
  std::mutex mu;
  std::condition_variable cv_job, cv_free;
  std::vector<Job> jobs;            // FIFO (few entries)
  std::vector<std::vector<uint8_t>> store;
  std::vector<uint8_t*> free_bufs;
  std::vector<std::thread> th;
  bool quit = false;
  int write_rc = RT_OK;
  std::string write_err;
  PngWriters(unsigned W, unsigned n_buffers, const Anim& a, AnimStats* stats) : store(n_buffers, frame_buffer(a.r.sc)) {
    for (auto& b : store) free_bufs.push_back(b.data());
    const uint32_t w = a.r.sc->width, h = a.r.sc->height;
    for (unsigned i = 0; i < W; ++i)
      th.emplace_back([this, &a, w, h, stats]() {
        for (;;) {
          Job j;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv_job.wait(lk, [&] { return quit || !jobs.empty(); });
            if (jobs.empty()) return;
            j = jobs.front(); jobs.erase(jobs.begin());
          }
          const auto t0 = Clock::now();
          const int rc = rt_png_write_rgb8(a.frame_name(j.frame).c_str(), j.px, w, h);
          const double ms = ms_since(t0);
          { std::lock_guard<std::mutex> lk(stats->mu); if (j.frame < (int)stats->png_ms.size()) stats->png_ms[j.frame] = ms; }
          std::lock_guard<std::mutex> lk(mu);
          if (rc != RT_OK && write_rc == RT_OK) { write_rc = rc; write_err = rt_host_last_error(); }
          free_bufs.push_back(j.px);
          cv_free.notify_one();
        }
      });
  }
  uint8_t* take_buffer() {  // blocks while every buffer is in flight or waiting for its PNG
    std::unique_lock<std::mutex> lk(mu);
    cv_free.wait(lk, [&] { return !free_bufs.empty(); });
    uint8_t* b = free_bufs.back(); free_bufs.pop_back();
    return b;
  }
  void give_buffer(uint8_t* b) { std::lock_guard<std::mutex> lk(mu); free_bufs.push_back(b); }
  void push(int frame, uint8_t* px) { { std::lock_guard<std::mutex> lk(mu); jobs.push_back({frame, px}); } cv_job.notify_one(); }
  bool failed() { std::lock_guard<std::mutex> lk(mu); return write_rc != RT_OK; }
  void finish() {  // every frame handed over is on disk, or has failed
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv_job.notify_all();
    for (auto& t : th) t.join();
    th.clear();
  }
};
// Several frames' PNGs are written at once, each by a FEW band threads: four writers x 8 threads keep up with the reference's 0.9 ms
// test-scene frames (one writer x 32 threads: 1.2 ms per PNG = slower than the kernel; three writers x 32 threads each: slower
// still, the threads of three PNGs at once — profiles/r06_run1_anim_writers.log).  RT_ANIM_WRITERS / RT_PNG_THREADS override.
unsigned anim_writers() {
  const char* e = std::getenv("RT_ANIM_WRITERS");
  const long v = e ? std::strtol(e, nullptr, 10) : 4;
  const unsigned w = v < 1 ? 1u : (v > 16 ? 16u : (unsigned)v);
  if (w > 1) setenv("RT_PNG_THREADS", "8", 0);
  return w;
}

// RT_ANIM=sharded (default): every frame SHARDED over the RT_GPUS devices (rt_hip_group_*), frames pipelined two deep: frame f+1 is
// submitted before frame f is collected, so f's gather + de-interleave + device-to-host copy run under f+1's kernels, and f's PNG is
// encoded on the writer threads (RT_ANIM_WRITERS, default 4) meanwhile.  2 + W host buffers: two frames in flight + one per writer.
// A group refuses an update while a frame is in flight, so with --shutter or --flat-frames frame f is collected before the scene moves
// for f + 1; its PNG is still written while f + 1 renders, and the next frame's file is read while the frame renders.
// p: frame 0's flat primitives, if any.
int animate_sharded(Anim& a, Pose& p) {
  RtHipGroup* hs = nullptr;
  const auto t_create = Clock::now();
  int rc = create_group(a.r, &hs);
  if (rc != RT_OK) return render_failed(rc);
  (void)rt_hip_group_set_option(hs, "prepare_host_output", 2);  // (pinned staging for the two frames in flight + the copy path, at set-up: not inside the first submit)
  if (a.r.o.flat_rebuild > 0 && (rc = rt_hip_group_set_option(hs, "flat_build", 1)) != RT_OK) { rt_hip_group_destroy(hs); return render_failed(rc); }
  const auto t_begin = Clock::now();
  const unsigned W = anim_writers();
  AnimStats stats(a.frames);
  PngWriters writers(W, 2 + W, a, &stats);
  int status = 0;
  std::vector<uint8_t*> in_flight;  // oldest first
  int submitted = 0, collected = 0;
  auto finish_oldest = [&]() -> bool {  // collect frame `collected`, print its two lines, hand its pixels to the PNG writers
    RtStats st{};
    const auto t0 = Clock::now();
    const int rc = rt_hip_group_collect(hs, &st);
    const auto t1 = Clock::now();
    stats.host_us[2] += ms_between(t0, t1) * 1e3;
    if (rc != RT_OK) { status = render_failed(rc); return false; }
    stats.frame(a, collected, st);
    writers.push(collected, in_flight.front());
    in_flight.erase(in_flight.begin());
    stats.host_us[3] += ms_since(t1) * 1e3;
    if (writers.failed()) return false;
    collected++;
    return true;
  };
  const bool scene_moves = p.flats || a.r.o.shutter >= 0.0;
  std::string flats_why;  // --flat-frames: what was wrong with a frame's file
  for (int f = 0; f < a.frames && status == 0 && !writers.failed(); ++f) {
    const auto t0 = Clock::now();
    uint8_t* buf = writers.take_buffer();
    const auto t1 = Clock::now();
    bool ok = true;
    while (ok && scene_moves && collected < submitted) ok = finish_oldest();  // (frame f - 1 is collected first, its PNG overlaps)
    if (!ok) { writers.give_buffer(buf); break; }
    a.view(f, p);
    rc = apply(hs, p);
    if (rc == RT_OK) rc = rt_hip_group_submit(hs, buf);
    stats.host_us[0] += ms_between(t0, t1) * 1e3;
    stats.host_us[1] += ms_since(t1) * 1e3;
    if (rc != RT_OK) { status = render_failed(rc); writers.give_buffer(buf); break; }
    in_flight.push_back(buf);
    submitted++;
    if (f + 1 < a.frames && !(flats_why = a.flats(f + 1, p)).empty()) break;  // (the next frame's file is read and checked while this frame renders)
    if (submitted - collected == 2 && !finish_oldest()) break;
  }
  while (status == 0 && !writers.failed() && collected < submitted && finish_oldest()) {}
  if (!flats_why.empty()) { std::fprintf(stderr, "%s\n", flats_why.c_str()); status = 101; }
  writers.finish();
  stats.report("sharded", collected, rt_hip_group_size(hs), W, ms_since(t_begin) / 1e3, ms_between(t_create, t_begin));
  rt_hip_group_destroy(hs);
  if (writers.write_rc != RT_OK) status = write_failed(writers.write_err.c_str());
  return status;
}

// Denoised animation (`--frames N --orbit DEG [--shutter S] --denoise`): the frames of the animation modes, each
// tracing a sample range of its own, blended with the previous frame's history where the first-hit surface was on screen one frame ago
// and filtered spatially (rt_hip_render_frame_temporal_to_host, RT_DENOISE_ITERATIONS iterations) on one resident scene.  The turn per
// frame must be named: --orbit is required (0 keeps the camera still).  Frame 0 is the `--denoise` one-shot frame, byte for byte.
// Frame f's PNG is encoded on the writer threads while frame f + 1 renders (1 + W host buffers: the frame being rendered + one per
// writer).  One GPU: RT_GPUS > 1 is refused.
// `--temporal-surface` (only in this mode) turns on surface tracking: moved spheres keep their history, Metal and Glass
// pixels get the floor `--temporal-alpha-specular B` on alpha (default RT_TEMPORAL_SURFACE_ALPHA_SPECULAR; needs --temporal-surface).
// `--temporal-alpha A` (only in this mode) sets alpha_min, the floor everywhere else (default RT_TEMPORAL_ALPHA_MIN, with
// --temporal-surface RT_TEMPORAL_SURFACE_ALPHA_MIN).  A and B lie in [0, 1]; anything else: the usage line.
int animate_temporal(Anim& a) {
  const cli::Options& o = a.r.o;
  RtHipScene* hs = nullptr;
  const auto t_create = Clock::now();
  int rc = create_scene(a.r, 0, &hs);
  if (rc == RT_OK && (o.t_surface || o.t_alpha >= 0.0)) {
    const float a_min = o.t_alpha >= 0.0 ? (float)o.t_alpha : (o.t_surface ? RT_TEMPORAL_SURFACE_ALPHA_MIN : RT_TEMPORAL_ALPHA_MIN);
    rc = rt_hip_temporal_configure(hs, a_min, RT_TEMPORAL_N_MAX, RT_TEMPORAL_TAU_NORMAL, RT_TEMPORAL_TAU_ALBEDO, RT_TEMPORAL_TAU_INV_DEPTH);
    if (rc == RT_OK && o.t_surface) rc = rt_hip_temporal_surface(hs, 1, o.t_alpha_specular >= 0.0 ? (float)o.t_alpha_specular : RT_TEMPORAL_SURFACE_ALPHA_SPECULAR);
  }
  if (rc != RT_OK) return render_failed(rc);
  const auto t_begin = Clock::now();
  const unsigned W = anim_writers();
  AnimStats stats(a.frames);
  PngWriters writers(W, 1 + W, a, &stats);
  Pose p;
  int status = 0, done = 0;
  for (int f = 0; f < a.frames && status == 0 && !writers.failed(); ++f) {
    uint8_t* buf = writers.take_buffer();
    a.pose(f, p);  // (no --flat-frames in this mode: nothing to read, nothing that fails)
    rc = apply(hs, p);
    RtStats st{};
    if (rc == RT_OK) rc = rt_hip_render_frame_temporal_to_host(hs, (uint32_t)f, RT_DENOISE_ITERATIONS, buf, &st);
    if (rc != RT_OK) { status = render_failed(rc); writers.give_buffer(buf); break; }
    stats.frame(a, f, st);
    writers.push(f, buf);
    done++;
  }
  writers.finish();
  stats.report("temporal", done, 1, W, ms_since(t_begin) / 1e3, ms_between(t_create, t_begin));
  rt_hip_scene_destroy(hs);
  if (writers.write_rc != RT_OK) status = write_failed(writers.write_err.c_str());
  return status;
}

// RT_ANIM=frames: the frames DISTRIBUTED over the devices — device g renders whole frames g, g + G, ... on its own resident
// scene and host thread (README.md:43-57 renders an animation one process per frame; this is that, with the scene loaded
// once per device).  No gather, no shard penalty, no per-frame synchronisation between devices; every frame is the bytes the
// sharded mode produces (Philox is addressed by pixel).  Per device the PNG of a frame is encoded while the next one renders: one
// writer and two buffers each.
int animate_frames(Anim& a, unsigned G) {
  const int ndev = rt_hip_device_count();
  const char* emu = std::getenv("RT_GPUS_EMULATE");
  if (ndev <= 0) { std::fprintf(stderr, "render failed: %s\n", rt_strerror(RT_ERR_NO_DEVICE)); return 101; }
  if (G > (unsigned)ndev && !(emu && emu[0] == '1')) {
    std::fprintf(stderr, "render failed: RT_GPUS = %u but only %d device(s) visible\n", G, ndev);
    return 101;
  }
  std::mutex out_mu;
  std::vector<int> status(G, 0);
  AnimStats stats(a.frames);
  const auto t_begin = Clock::now();
  std::vector<std::thread> th;
  for (unsigned g = 0; g < G; ++g)
    th.emplace_back([&, g]() {
      auto say = [&](auto&& print) { std::lock_guard<std::mutex> lk(out_mu); print(); };  // (one device's lines at a time)
      RtHipScene* hs = nullptr;
      int rc = create_scene(a.r, (int)(g % (unsigned)ndev), &hs);
      if (rc == RT_OK && a.r.o.flat_rebuild > 0 && (rc = rt_hip_set_option(hs, "flat_build", 1)) != RT_OK) { rt_hip_scene_destroy(hs); hs = nullptr; }
      if (rc != RT_OK) { say([&] { status[g] = render_failed(rc); }); return; }
      PngWriters writers(1, 2, a, &stats);
      Pose p;
      for (int f = (int)g; f < a.frames && !writers.failed(); f += (int)G) {
        const std::string why = a.pose(f, p);
        if (!why.empty()) { say([&] { std::fprintf(stderr, "%s\n", why.c_str()); status[g] = 101; }); break; }
        uint8_t* buf = writers.take_buffer();
        rc = apply(hs, p);
        RtStats st{};
        if (rc == RT_OK) rc = rt_hip_render_to_host(hs, buf, &st);
        if (rc != RT_OK) { say([&] { status[g] = render_failed(rc); }); writers.give_buffer(buf); break; }
        say([&] { stats.frame(a, f, st); });
        writers.push(f, buf);
      }
      writers.finish();
      if (writers.write_rc != RT_OK) say([&] { status[g] = write_failed(writers.write_err.c_str()); });
      rt_hip_scene_destroy(hs);
    });
  for (auto& t : th) t.join();
  stats.report("frames", a.frames, G, 1, ms_since(t_begin) / 1e3, 0.0);
  for (int s : status) if (s) return s;
  return 0;
}

// Animation (SURVEY §8f "animation driver"): `raytracer <config_file> <output_prefix> --frames N [--orbit DEG]` renders N frames to
// `<output_prefix>_%03d.png` — the file naming main.rs:17 keeps commented out and README.md:43-57 / "Make animation" feed to ffmpeg —
// turning the camera around look_at by DEG per frame (default 360/N).  The scene is uploaded once and stays in HBM; the PNG of frame i
// is encoded on writer threads while the GPU renders frame i+1.  With RT_GPUS=G every frame is sharded over the G devices
// (RT_ANIM=sharded, default), or the frames are distributed over the devices, each rendering whole frames (RT_ANIM=frames);
// RT_STATS=1 prints frames per second and the per-frame kernel / frame / PNG times to stderr (one JSON line).
//
// Moving spheres from frame to frame (`--frames N --shutter S`, 0 <= S <= 1): a sphere's "center" -> "center1" is its
// path over the whole animation instead of over one exposure; frame f is exposed from center + dv f / N to center + dv (f + S) / N
// (anim_path.h), S = 0 giving crisp spheres.  The resident scene's spheres are moved before every frame (rt_hip_group_update_spheres /
// rt_hip_scene_update_spheres: the grid is rebuilt on the GPU).  Only with --frames; without the flag every frame exposes the scene
// file's center -> center1.
//
// Moving flat primitives from frame to frame (`--frames N --flat-frames PREFIX`): frame f takes its flat primitives from the
// scene file PREFIX%03d.json (only its quads, boxes, triangles and meshes are used; count, shapes and materials must be the base file's —
// anything else, or an unreadable file, ends the run with a message that names the frame).  The resident scene's flat primitives are moved
// before every frame (rt_hip_group_update_flats / rt_hip_scene_update_flats: the structure of --flat-bvh is refit on the GPU).  Combines
// with --orbit, --shutter, --flat-bvh, RT_GPUS and RT_ANIM=frames; without --frames, or with --denoise, --passes or --adaptive: the usage line.
// `--flat-rebuild K` (only with --flat-frames, K >= 1): the update of every K-th frame (f % K == 0, f > 0) carries
// RT_UPDATE_FLATS_REBUILD and the scene's option "flat_build" is 1 — the structure is built anew on the device instead of refit.  The scene
// must have the structure.  A rebuild changes how fast the frames trace, never what they are: the PNGs are those of the run without the flag.
int animate(const Run& r) {
  Anim a(r);
  if (r.o.mode == cli::DENOISED_ANIMATION) return animate_temporal(a);
  Pose first;
  if (a.flat_files.on()) {  // (frame 0's file is read and checked before anything is created on a device)
    uint32_t n_quads = 0;
    const RtQuad* quads = rt_scene_quads(r.sf, &n_quads);
    if (!n_quads) { std::fprintf(stderr, "--flat-frames: the scene has no flat primitive\n"); return 101; }
    a.flat_files.base.assign(quads, quads + n_quads);
    uint32_t n_normals = 0;
    if (const double* nr = rt_scene_flat_normals(r.sf, &n_normals)) a.flat_files.base_normals.assign(nr, nr + 9 * (size_t)n_normals);
    a.flat_files.moved = rt_scene_flat_motion(r.sf, nullptr) != nullptr;
    a.flat_files.lit = rt_scene_flat_emit(r.sf, nullptr) != nullptr;
    const std::string why = a.flats(0, first);
    if (!why.empty()) { std::fprintf(stderr, "%s\n", why.c_str()); return 101; }
    if (r.o.flat_rebuild > 0 && !(r.o.flat_bvh || rt_scene_flat_bvh(r.sf))) {
      std::fprintf(stderr, "--flat-rebuild: the scene has no structure over its flat primitives (\"flat_bvh\": true in the file, or --flat-bvh)\n");
      return 101;
    }
  }
  const char* mode = std::getenv("RT_ANIM");
  if (mode && !std::strcmp(mode, "frames")) {
    const unsigned G = (unsigned)gpus_asked(r.sc);
    if (G < 1 || G > 1024) { std::fprintf(stderr, "render failed: RT_GPUS must be a positive device count\n"); return 101; }
    return animate_frames(a, G);
  }
  if (mode && std::strcmp(mode, "sharded")) { std::fprintf(stderr, "RT_ANIM must be sharded (default) or frames\n"); return 101; }
  return animate_sharded(a, first);
}

// The HIP runtime takes 50 - 200 ms to come up (its first call) — as long as the reference's three 2 - 3 MP JPEG textures take to
// decode.  A thread makes that first call while the main thread reads and parses the scene (at 13 ms a frame the host
// pipeline IS the wall time).
std::thread g_hip_init;
double g_hip_init_ms = 0.0;
void start_hip_init() {
  g_hip_init = std::thread([]() {
    const auto t0 = Clock::now();
    const int n = rt_hip_device_count();
    // ... and the context + code object of every device the run will use (RT_GPUS, default 1): rt_hip_scene_create finds them up
    const long want = gpus_asked(nullptr);
    std::vector<std::thread> per_device;  // (side by side: a context takes ~30 ms each)
    for (int d = 1; d < n && d < want; ++d) per_device.emplace_back([d]() { (void)rt_hip_device_warm(d); });
    if (n > 0) (void)rt_hip_device_warm(0);
    for (auto& t : per_device) t.join();
    g_hip_init_ms = ms_since(t0);
  });
}
void join_hip_init() { if (g_hip_init.joinable()) g_hip_init.join(); }

// rt_render_rgb8 for a scene with a thin lens, moving spheres or quads (RtScene carries none of them): the same one-frame group, with the
// lens camera c (rt_camera_derive_lens; null: RtScene's pinhole), the spheres' centres at shutter close and the quads of the scene file
int render_group_rgb8(const Run& r, const double* c, uint8_t* out_rgb8, RtStats* stats) {
  const auto t0 = Clock::now();
  RtHipGroup* g = nullptr;
  int rc = create_group(r, &g);
  if (rc != RT_OK) return rc;
  (void)rt_hip_group_set_option(g, "tile_order", 1);  // (one frame: no later frame could use a learned order — rt_render_rgb8's setting)
  if (c) {
    rc = rt_hip_group_set_camera(g, c, c + 3, c + 6, c + 9);
    if (rc == RT_OK) rc = rt_hip_group_set_lens(g, c + 13, c + 16, c[19]);
  }
  if (rc == RT_OK) rc = rt_hip_group_set_option(g, "prepare_host_output", 1);
  const double setup_ms = ms_since(t0);
  if (rc == RT_OK) rc = rt_hip_group_render_to_host(g, out_rgb8, stats);
  if (rc == RT_OK && stats) stats->setup_ms = setup_ms;
  rt_hip_group_destroy(g);
  return rc;
}

// The reference's run: one frame, one PNG.  RtScene has no lens, no moving spheres and no quads, so the one-shot frame of a scene file
// with any of them goes through a one-frame group, not rt_render_rgb8.
int one_shot(const Run& r, Clock::time_point t_main) {
  const RtScene* sc = r.sc;
  const double load_done_ms = ms_since(t_main);
  std::printf("\nRendering %s\n", r.o.output);  // main.rs:18
  std::vector<uint8_t> pixels = frame_buffer(sc);
  RtStats st{};
  const auto t_hip = Clock::now();
  join_hip_init();  // (what of the runtime's start-up the load did not cover)
  const double hip_wait_ms = ms_since(t_hip), hip_init_ms = g_hip_init_ms;
  double cam_lens[20];
  const bool lens = lens_camera(r.sf, cam_lens);
  uint32_t n_quads = 0;
  (void)rt_scene_quads(r.sf, &n_quads);
  int rc = lens || rt_scene_motion(r.sf) || n_quads ? render_group_rgb8(r, lens ? cam_lens : nullptr, pixels.data(), &st) : rt_render_rgb8(sc, pixels.data(), &st);
  if (rc != RT_OK) return render_failed(rc);
  std::printf("Frame time: %lldms\n", (long long)st.frame_ms);  // raytracer.rs:263
  const auto t_png = Clock::now();
  rc = rt_png_write_rgb8(r.o.output, pixels.data(), sc->width, sc->height);  // raytracer.rs:265
  const double png_ms = ms_since(t_png);
  if (std::getenv("RT_STATS")) {  // where a drop-in user's wall time goes: main() entered -> PNG on disk
    double lt[4] = {0, 0, 0, 0};
    rt_scene_load_timings(r.sf, lt);
    std::fprintf(stderr, "{\"samples\":%llu,\"segments\":%llu,\"sphere_tests\":%llu,\"exact_tests\":%llu,\"n_gpus\":%u,\"kernel_ms\":%.3f,"
                         "\"gather_ms\":%.3f,\"frame_ms\":%.3f,\"setup_ms\":%.3f,\"msamples_per_s\":%.3f,"
                         "\"load_ms\":%.3f,\"read_ms\":%.3f,\"json_ms\":%.3f,\"jpeg_ms\":%.3f,\"hip_init_ms\":%.3f,\"hip_wait_ms\":%.3f,\"png_ms\":%.3f,\"main_ms\":%.3f,"
                         "\"group_us\":[%.1f,%.1f,%.1f,%.1f,%.1f,%.1f,%.1f,%.1f],\"setup_profile\":%s}\n",
                 (unsigned long long)st.samples, (unsigned long long)st.segments, (unsigned long long)st.sphere_tests,
                 (unsigned long long)st.exact_tests, st.n_gpus_used, st.kernel_ms, st.gather_ms, st.frame_ms, st.setup_ms,
                 st.samples / (st.kernel_ms * 1e3), load_done_ms, lt[0], lt[1], lt[2], hip_init_ms, hip_wait_ms, png_ms, ms_since(t_main),
                 st.group_us[0], st.group_us[1], st.group_us[2], st.group_us[3], st.group_us[4], st.group_us[5], st.group_us[6], st.group_us[7],
                 rt_hip_setup_profile());
  }
  return rc != RT_OK ? write_failed(rt_host_last_error()) : 0;
}

// the modes that render on one GPU, when the run asks for more (0: go on)
int refuse_many_gpus(const Run& r) {
  const bool animation = r.o.mode == cli::ANIMATION, one = r.o.mode == cli::ONE_SHOT;
  if (animation || one || gpus_asked(r.sc) <= 1) return 0;
  const char* flag = r.o.denoise ? "denoise" : (r.o.adaptive ? "adaptive" : "passes");
  const char* form = r.o.denoise ? "denoised" : (r.o.adaptive ? "adaptive" : "progressive");
  std::fprintf(stderr, "--%s renders on one GPU: unset RT_GPUS (the multi-GPU group calls have no %s form)\n", flag, form);
  return 101;
}
int dispatch(const Run& r, Clock::time_point t_main) {
  if (r.o.passes > 0 && (unsigned long)r.o.passes > r.sc->samples_per_pixel) return usage(r.o);
  if (const int status = refuse_many_gpus(r)) return status;
  if (r.o.mode == cli::ONE_SHOT) return one_shot(r, t_main);
  join_hip_init();
  switch (r.o.mode) {
    case cli::ADAPTIVE: return adaptive(r);
    case cli::ANIMATION: case cli::DENOISED_ANIMATION: return animate(r);
    default: return progressive(r);  // --passes K, --denoise, or both
  }
}
}  // namespace

int run(int argc, char** argv) {
  const auto t_main = Clock::now();
  const cli::Options o = cli::parse(argc, argv);
  if (o.mode == cli::USAGE) return usage(o);
  // One frame per process (the reference's way, main.rs:7-20): the runtime's copy engines are hardware queues it creates at
  // their FIRST use — 7.8 ms for the first host-to-device copy, 7.8 ms for the first device-to-host copy on MI355X
  // (tools/microbench/setup_costs.hip) — to move 80 KB of tables in and 2.9 MB of pixels out once.  With HSA_ENABLE_SDMA=0 the
  // runtime copies with kernels on the compute queue that exists anyway (same copy times at these sizes, measured).  Only here:
  // an animation keeps the engines — its copies run UNDER the next frame's kernel, which leaves a copy kernel no registers.
  // A value the user set is left alone.
  if (o.frames == 0) setenv("HSA_ENABLE_SDMA", "0", 0);
  start_hip_init();
  RtSceneFile* sf = nullptr;
  if (rt_scene_load_file(o.config, &sf) != RT_OK) {
    std::fprintf(stderr, "%s\n", rt_host_last_error());
    return 101;
  }
  const Run r{o, sf, rt_scene_get_mut(sf)};
  if (const char* seed = std::getenv("RT_SEED")) r.sc->seed = std::strtoull(seed, nullptr, 0);
  const int status = dispatch(r, t_main);
  rt_scene_free(sf);
  return status;
}

// Everything the process owes the world is on disk or in the pipe when run() returns: stdout / stderr are flushed and the process
// ends WITHOUT the HIP runtime's tear-down (static destructors: tens of milliseconds the reference's binary does not have).
// RT_FAST_EXIT=0 takes the ordinary way out.
int main(int argc, char** argv) {
  const int status = run(argc, argv);
  join_hip_init();
  std::fflush(stdout);
  std::fflush(stderr);
  const char* fe = std::getenv("RT_FAST_EXIT");
  if (!(fe && fe[0] == '0')) std::_Exit(status);
  return status;
}
