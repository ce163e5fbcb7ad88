// rt_hip_api.hip — extern "C" entry points of librt_hip.so (include/rt_abi.h): scene upload
// to HBM, megakernel launch on a caller-supplied stream, HIP-event timing, counters.
// This is the drop-in for the rayon loop at reference raytracer.rs:260-262.  There is no CPU
// path in this library: without a gfx950 device every call fails with RT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <optional>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rt_kernel.hip"
#include "rt_tables.h"
#ifdef RT_TEST_PROBES  // librt_hip_probe.so: the device probes and debug calls of include/rt_abi_test.h (test infrastructure)
#include "../../../include/rt_abi_test.h"
#include "../../../include/rt_abi_test_flat_motion.h"
#endif

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

#define RT_HIP_TRY(expr)                                                                            \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      return fail(RT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                   \
  } while (0)

// Wide tables have no kernel for media, solid textures or quads (rtk::kernel_key_valid): such a scene is refused where its tables are made.
int check_wide_tables(bool wide, bool media, bool solids, bool quads = false) {
  if (rtk::kernel_key_valid((wide ? rtk::KEY_WIDE : 0) | (media ? rtk::KEY_MEDIUM : 0) | (solids ? rtk::KEY_SOLID : 0) | (quads ? rtk::KEY_QUADS : 0))) return RT_OK;
  return fail(RT_ERR_UNSUPPORTED, std::string(media ? "participating media" : (solids ? "solid textures" : "quads")) + " in a scene with wide tables (more than 65 535 spheres)");
}

// Argument checks the entry points share.  Each returns RT_OK or the refusal it has recorded (fail): `if (const int refused = ...) return refused;`
// `p` is a multiple of `align` bytes, a power of two (null passes: what may be null is the caller's business)
int check_aligned(const void* p, uintptr_t align, const char* message) {
  return (reinterpret_cast<uintptr_t>(p) & (align - 1u)) ? fail(RT_ERR_INVALID, message) : RT_OK;
}
// samples [begin, begin + count) of a pixel fit the exact sums: 2^-40 fixed point in 64 bits (rt_core.h ACCUM_MAX_SAMPLES)
int check_samples(uint64_t begin, uint64_t count, const char* holder = "an accumulator holds ") {
  return begin + count > rtc::ACCUM_MAX_SAMPLES ? fail(RT_ERR_UNSUPPORTED, std::string(holder) + "at most 2^23 - 1 samples per pixel") : RT_OK;
}
// does the output range lie over one of the input ranges?  (it would be read by other threads while it is written; a null output: no)
struct Range { const void* p; size_t bytes; };
bool overlaps(Range out, std::initializer_list<Range> inputs) {
  const uintptr_t o0 = (uintptr_t)out.p, o1 = o0 + out.bytes;
  for (const Range& in : inputs)
    if (o0 && (uintptr_t)in.p < o1 && o0 < (uintptr_t)in.p + in.bytes) return true;
  return false;
}

}  // namespace

struct RtHipScene;
namespace { int warm_up(RtHipScene* s); }

// Where set-up time goes (rt_hip_setup_profile): the stages of the most recent scene / group creation and one-shot render of
// this process, in milliseconds — rank 0's scene and the group's own work; other ranks' scenes are created beside it.
namespace rtp {
std::mutex g_mu;
std::vector<std::pair<std::string, double>> g_stages;
thread_local bool tl_record = true;     // (the group's upload threads of ranks >= 1 switch it off)
thread_local bool tl_in_group = false;  // a group is being created on this thread: its scene's stages are appended to the group's
                                        // (a scene created on its own starts a profile of its own: the list never grows without bound)
thread_local std::string tl_text;
void reset() { std::lock_guard<std::mutex> lk(g_mu); g_stages.clear(); }
void add(const char* name, double ms) { if (!tl_record) return; std::lock_guard<std::mutex> lk(g_mu); g_stages.emplace_back(name, ms); }
struct Clock {   // mark("x") books the time since the previous mark under x
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(const char* name) {
    const auto n = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(n - t).count();
#ifdef RT_DEV_KNOBS  // (development: RT_GROUP_TRACE=1 prints every stage of every rank as it ends, to stderr)
    static const bool trace = std::getenv("RT_GROUP_TRACE") != nullptr;
    if (trace) std::fprintf(stderr, "[rt] %s %.3f ms\n", name, ms);
#endif
    add(name, ms);
    t = n;
  }
};
// how a scene's creation or update starts: with a profile of its own, unless a group is being created
Clock begin() { if (!tl_in_group) reset(); return Clock(); }
}  // namespace rtp
extern "C" const char* rt_hip_setup_profile(void) {
  std::lock_guard<std::mutex> lk(rtp::g_mu);
  std::string& s = rtp::tl_text;
  s = "{";
  char buf[96];
  for (size_t i = 0; i < rtp::g_stages.size(); ++i) {
    std::snprintf(buf, sizeof buf, "%s\"%s\":%.3f", i ? "," : "", rtp::g_stages[i].first.c_str(), rtp::g_stages[i].second);
    s += buf;
  }
  s += "}";
  return s.c_str();
}

constexpr uint32_t RT_TIMELINE_WAVES = 8192;  // profile builds: {start, end} wall clock per wave behind the counters

// One device allocation, owned: freed with its owner (on the current device: the owner sets it).  ensure() is the only place that
// frees an existing buffer to allocate a larger one.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }  // (what this one held is freed with `o`)
  ~DevBuf() { if (p) (void)hipFree(p); }
  template <typename T = void> T* get() const { return static_cast<T*>(p); }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  // At least `bytes`; *grew: it was (re)allocated, its contents are undefined.  Before an existing buffer is freed the work that may
  // still read it has finished: the whole device's, or only `stream`'s where the caller knows that is the one stream using it.
  // Runs only when a buffer grows — never per frame in steady state.
  int ensure(size_t bytes, bool* grew = nullptr, std::optional<hipStream_t> stream = std::nullopt) {
    if (grew) *grew = false;
    if (bytes <= cap) return RT_OK;
    if (p) {
      RT_HIP_TRY(stream ? hipStreamSynchronize(*stream) : hipDeviceSynchronize());
      (void)hipFree(p);
      p = nullptr; cap = 0;
    }
    RT_HIP_TRY(hipMalloc(&p, bytes));
    cap = bytes;
    if (grew) *grew = true;
    return RT_OK;
  }
};

enum class Moved { spheres, flats };  // what an update replaced in a resident scene (adopt_tables)

struct RtHipScene {
  int device = 0;
  // What rt_hip_scene_create builds, once: shared by the scene and its views (rt_hip_scene_clone_view), freed with the last of them.
  // The tables an update replaces come in generations of one type: `live` is what the kernels read, `spare` what the next update builds
  // into and swaps in when it has succeeded — the old tables are the update after's spares, a steady animation allocates nothing.
  struct Resident {
    int device = 0;
    bool has_lights = false, simple_colour = false;
    int num_cus = 0;
    size_t lds_cap = 0;      // dynamic LDS a workgroup may ask for on this device
    // The spheres, and what rt_hip_scene_update_spheres moves them with.
    struct Spheres {
      struct Tables {          // the geometry and the product grid (variant 0) over it
        DevBuf geom, cell_word, cell_items, large, large_geom;
        rtc::GridDesc grid{};
        // motion blur: [n][4] dv per sphere (rt_tables.h HostTables::motion).  It counts only while n_moving: static tables own whatever
        // buffer the swap left them (none, or an older generation's rows), and every reader asks n_moving first (Resident::point, rt_hip_scene_table)
        DevBuf motion;
        uint32_t n_moving = 0;
      } live, spare;
      struct Scratch { DevBuf centre, plan_large, range, lflag, lpos, count, start, cursor, block_sum, counts, raw_items, raw_cell; } scratch;  // the device builder's
      DevBuf all;              // 0..n-1: the `large` list of the brute-force arm (variant 1)
      // on the host: the spheres at their current centres (the host plans the next grid from them) and a second copy the next centres are
      // written into; the plan; the staging of the motion upload, kept like the texels below
      std::vector<RtSphere> spheres, next_spheres;
      rtc::GridPlan plan;
      std::vector<double> keep_motion;
      // each sphere's centre at shutter time 0.5 of the live tables, c + (c1 - c) * 0.5 in f64 ([n][3]; rt_hip_temporal_surface's displacement)
      std::vector<double> mid;
      void set_mid(const std::vector<double>& motion) {
        mid.resize(3 * spheres.size());
        for (size_t i = 0; i < spheres.size(); ++i)
          for (int k = 0; k < 3; ++k) mid[3 * i + k] = spheres[i].center[k] + (motion.empty() ? 0.0 : motion[4 * i + k]) * 0.5;
      }
    } sph;
    // The flat primitives (quads; triangles, §21), the structure over them (§22: only in a scene that came from
    // rt_hip_scene_create_flats_bvh) and what rt_hip_scene_update_flats (§24) moves them with.  The calls that change them are in
    // rt_hip_flats.hip; all of them go from the live generation to the next through one function (flats_go_live, §24 "One update path"),
    // which is handed a HeaderState: what the next generation's header names.
    struct Flats {
      struct Tables {
        // [n_quads] RtQuadRec, their materials are records n_spheres + k of `mat` and `matc`; while the header names anything — the structure
        // or a table of normals, motion or images (HeaderState::slot) — one buffer, the FlatBvhHeader in front of the records
        // (Flats::first_rec).  Unallocated without quads.
        DevBuf rec;
        DevBuf nodes, order;   // the structure: [n_nodes] FlatNode and [n_quads] the order table its leaves index
      } live, spare;           // (a refit keeps the live order table: only a rebuild swaps it)
      DevBuf lim;              // [n_quads] the limit of alpha + beta per entry; unallocated in a scene without a triangle
      uint32_t n_quads = 0, n_tris = 0, n_nodes = 0;  // (n_nodes: of the live structure; 0: none, every segment scans the records)
      // shading normals (rt_hip_scene_set_flat_normals): [n_quads][9] the records of rt_flat_normal.h and the table the next
      // call builds into; n_normals: the entries that have normals, 0: no table — the scene is one that never had any
      DevBuf normals, normals_spare;
      uint32_t n_normals = 0;
      // motion within the frame (rt_hip_scene_set_flat_motion): [n_quads][4] the records of rt_flat_motion.h and the table the
      // next call or update builds into; n_moving: the entries that move, 0: no table — the scene is one that never had any.  still: the
      // all -0.0 dv table [n_spheres][4] the MOTION kernels read in a scene whose only movers are flat primitives (§14: a static sphere's bits).
      DevBuf motion, motion_spare, still;
      uint32_t n_moving = 0;
      // images (rt_hip_scene_set_flat_images): [n_quads] the records of rt_flat_image.h and the table the next call builds into;
      // n_images: the entries that have one, 0: no table — the scene is one that never had any.  tex_table: what the prepare kernel knows of
      // the scene's textures ([n_textures] RtFlatImageTex, uploaded at creation); tex4_dev: Resident::tex4, which the header names beside the records
      DevBuf images, images_spare, tex_table;
      uint32_t n_images = 0, n_textures = 0;
      const uint32_t* tex4_dev = nullptr;
      // what a refit needs of the structure as built (rt_flat_build.h FlatTopology), on the device and on the host: topo's vectors are the staging of their uploads
      DevBuf boxed, leaves, levels;
      rtc::FlatTopology topo;
      // the device code's: the geometry as uploaded, a box per entry, the status block; the device build's (§26) items, range extents, sort storage
      struct Scratch { DevBuf quv, box, status, item, extent, sort_tmp, move, rec_tmp, kind; } scratch;
      // the device build starts from the boxed entries in index order: resident from the first device build after each host build on
      DevBuf start;
      std::vector<uint32_t> keep_start;
      bool start_ready = false;
      uint32_t device_builds = 0;   // order tables built on the device since creation
      // on the host: the limits (a rebuild runs build_flat_bvh) and the staging of a rebuild's uploads, kept like the texels below
      std::vector<double> host_lim, keep_quv;
      std::vector<rtc::FlatNode> keep_nodes;
      std::vector<uint32_t> keep_order;
      rtc::FlatBvhHeader keep_header{};   // (the staging of the header's upload: written by flats_go_live alone)
      uint32_t refits = 0;     // the updates applied by refit since the structure was last built
      // What a generation's header names: the structure's nodes and order table and the tables of normals, motion and images, each with the
      // count that says whether it is there, and the buffer behind it — a live one or the spare an update built into.  slot(): the record
      // slots the header takes in front of the records: one while it names anything, none in a scan scene without a table.
      struct HeaderState {
        uint32_t n_nodes = 0, n_normals = 0, n_moving = 0, n_images = 0;
        const DevBuf *nodes = nullptr, *order = nullptr, *normals = nullptr, *motion = nullptr, *images = nullptr;
        uint32_t slot() const { return (n_nodes || n_normals || n_moving || n_images) ? 1u : 0u; }
      };
      HeaderState state() const { return {n_nodes, n_normals, n_moving, n_images, &live.nodes, &live.order, &normals, &motion, &images}; }  // the live generation's
      // the first record of a generation as the kernels see it (DevScene::quads.rec): behind the header, where there is one
      RtQuadRec* first_rec(const Tables& t) const { return t.rec.get<RtQuadRec>() + state().slot(); }
      const double* dev_lim() const { return n_tris ? lim.get<const double>() : nullptr; }
      // the header of the generation `st` describes, its records beginning at `rec`
      rtc::FlatBvhHeader header(const HeaderState& st, const RtQuadRec* rec, uint32_t id_base) const {
        rtc::FlatBvhHeader h{};
        h.nodes = st.nodes->get<const rtc::FlatNode>(); h.order = st.order->get<const uint32_t>();
        h.rec = rec; h.lim = dev_lim();
        h.n_nodes = st.n_nodes; h.n_quads = n_quads; h.id_base = id_base;
        h.normals = st.n_normals ? st.normals->get<const double>() : nullptr;
        h.motion = st.n_moving ? st.motion->get<const double>() : nullptr;
        h.images = st.n_images ? st.images->get<const RtFlatImageRec>() : nullptr;
        h.tex4 = st.n_images ? tex4_dev : nullptr;
        return h;
      }
    } flat;
    // Materials, lights, media, textures and sky: uploaded at creation, never replaced — but for emission (rt_hip_scene_set_flat_lights,
    // DESIGN.md §28), which rewrites the emitters' records of `mat` and `matc` and the light list: the Light spheres, then the emitters as
    // object ids n_spheres + k.  On the host for that: the flat primitives' records as created (what an entry is again when it stops
    // emitting), the Light spheres, and the emitters' entry indices in light order (empty: the scene is one that never had any).
    DevBuf mat, matc, lights;
    std::vector<rtc::SphereMat> keep_flat_mat;
    std::vector<rtc::MatCore> keep_flat_matc;
    std::vector<uint32_t> sphere_lights, flat_lights;
    uint32_t n_lights() const { return (uint32_t)(sphere_lights.size() + flat_lights.size()); }
    DevBuf medium;           // participating media: [n] density per sphere, 0 = no medium (HostTables::medium); unallocated without media
    uint32_t n_media = 0;
    uint32_t n_solids = 0;   // solid textures: Checker and Noise spheres (and quads); their parameters are in the `mat` records
    DevBuf tex, sky, tex4, sky4;
    // The host copies of the BIG uploads (texels: 29 MB for the reference's test scene) live as long as the scene.  hipMemcpy from
    // pageable memory pins the source pages for the device (a userptr mapping the runtime caches); giving such memory back to
    // the OS (free -> munmap) fires the driver's MMU notifier, which EVICTS the process's hardware queues and restores them
    // 10 - 25 ms later — the next kernel launch waits for that.  Found in round 6 as a one-shot frame of the test scene whose
    // first launch started 20 ms late in two runs of three (profiles/r06_run5_first_launch_wait.log); with the buffers kept,
    // 12 of 12 runs start in 0.07 ms.  They are freed with the scene, when nothing waits for the queues.
    rtc::TexelVec keep_tex4, keep_sky4;
    std::vector<uint8_t> keep_tex_rgb8, keep_sky_rgb8;
    size_t texel_bytes = 0;
    // Point a scene's (or a view's) kernels at the live tables: every pointer and count of DevScene that follows from this struct.
    void point(rtc::DevScene& d) const {
      const Spheres::Tables& t = sph.live;
      d.grid = t.grid;
      d.geom = t.geom.get<const rtc::SphereGeom>(); d.cell_word = t.cell_word.get<const uint32_t>();
      d.cell_items = t.cell_items.get<const uint16_t>(); d.large = t.large.get<const uint32_t>();
      d.large_geom = t.large_geom.get<const rtc::SphereGeom>();
      // (§27: flat primitives that move select the MOTION kernels too; without a moving sphere those read the all -0.0 table)
      d.motion = t.n_moving ? t.motion.get<const double>() : (flat.n_moving ? flat.still.get<const double>() : nullptr);
      d.quads.rec = flat.n_quads ? flat.first_rec(flat.live) : nullptr; d.quads.lim = flat.dev_lim();
      d.n_quads = flat.n_quads;
      d.n_tris = flat.n_tris | (flat.n_nodes ? rtc::FLAT_BVH_BIT : 0u) |  // (§22: the bit says that the header lies in front of quads.rec[0])
                 (flat.n_normals ? rtc::FLAT_NORMALS_BIT : 0u) |            // (§25: ... and that it names a table of shading normals)
                 (flat.n_moving ? rtc::FLAT_MOTION_BIT : 0u) |              // (§27: ... and a table of motion records)
                 (flat_lights.empty() ? 0u : rtc::FLAT_LIGHTS_BIT) |        // (§28: the light list names emitting flat primitives)
                 (flat.n_images ? rtc::FLAT_IMAGES_BIT : 0u);               // (§29: the header names a table of image records and the texels)
      // (§28: the light count and what fill_dev_scene derives from it, by its operations: emission can change them after creation)
      d.n_lights = n_lights();
      d.light_thr[0] = 1.0 - (double)d.n_lights * 0.1;
      d.light_thr[1] = 1.0 - (double)d.n_lights * 0.05;
      d.mat = mat.get<const rtc::SphereMat>(); d.matc = matc.get<const rtc::MatCore>();
      d.lights = lights.get<const uint32_t>(); d.medium = n_media ? medium.get<const double>() : nullptr;
      d.tex = tex.get<const uint8_t>(); d.sky = sky.get<const uint8_t>();
      d.tex4 = tex4.get<const uint32_t>(); d.sky4 = sky4.get<const uint32_t>();
    }
    ~Resident() { (void)hipSetDevice(device); }  // (the buffers are freed after this body)
  };
  std::shared_ptr<Resident> res;
  RtScene host{};          // scalar fields only (pointers are not kept)
  rtc::DevScene dev{};     // device pointers filled in
  struct Options {         // what rt_hip_set_option sets (a view starts with its scene's)
    int variant = 0;
    int tile_log2 = -1;      // -1 = automatic; else tiles of 4^k pixels, k = 0..3
    int tile_shape = 0;      // 0: 2^k x 2^k squares (default: 0.9 % faster); 1: runs of 4^k pixels of one scanline (contiguous
                             // framebuffer bytes: HBM writes 10.9 -> 5.9 MiB per 1200x800 frame, profiles/r02_run8_*)
    int tile_affinity = 1;   // "tile_affinity" option: runs of tiles belong to one XCD's queue (framebuffer lines complete in one L2)
    int order_mode = 2;      // "tile_order" option: 0 top row first, 1 bottom row first, 2 deepest tiles of the previous frame first
                             // (a frame without a previous one: bottom row first)
    int force_lit = 0;       // "force_lit" option (diagnostics)
    int light_pool_cap = 0;  // "light_pool" option: cap on the light-frame pool of lit scenes (0 = automatic; tests shrink it to force repeats and overflows)
    int light_base_cap = 0;  // "light_base_pool" option: the same for the pool of colour-map bases
    int light_nest_pool = 1; // "light_nest_pool" option: 0 = nested light activations always go through the HBM overflow (tests)
    int chunk_spp = 0;       // 0 = automatic
    int tile_batch = 0;      // 0 = automatic; else tiles a workgroup takes from the queue per atomic, 1..64
    int flat_build = 0;      // "flat_build" option: who builds the order table when rt_hip_scene_update_flats is asked to rebuild: 0 the host, 1 the device
  } opt;

  // What a launch writes — each scene and view has its own.
  DevBuf counters;          // 4 counters + the work-queue cursor
  int cfg_key = -1; size_t cfg_lds = 0; int cfg_per_cu = 0;  // cached launch configuration
  DevBuf frame;             // framebuffer of rt_hip_render_to_host
  // What the scene DERIVES from its tables, camera and options lives in four structs by owner (`order` here; `prog`, `tp` and `ad` below), each
  // with the ONE member that drops it.  Who drops what: every entry is one call at the event's site, "-" means the event leaves it alone.
  //
  //   event                                                           order               prog       ad        tp
  //   rt_hip_set_camera, the same four vectors                        -                   reset()    -         -
  //   rt_hip_set_camera, another camera                               forget()            reset()    -         -
  //   rt_hip_set_lens, the same lens                                  -                   -          -         -
  //   rt_hip_set_lens, another lens                                   forget()            reset()    -         -
  //   option tile_order, tile_affinity                                forget()            -          -         -
  //   option seed, max_depth, accum_reset                             -                   reset()    -         -
  //   option samples_per_pixel and every other option                 -                   -          -         -
  //   rt_hip_scene_update_spheres, a view following (adopt_tables)    forget()            reset()    reset()   -
  //   rt_hip_scene_update_flats, a view following (adopt_tables)      forget()            reset()    reset()   reset()
  //   a launch whose OrderKey differs (launch_frame)                  forget(), new key   -          -         -
  //   rt_hip_scene_warm (+ launch bookkeeping as after creation)      forget(), no key    -          -         -
  //   rt_hip_temporal_surface (a real change), rt_hip_temporal_reset  -                   -          -         reset()
  //   a host form that failed, or whose buffer grew: its own state    -                   reset()    -         valid = false
  //
  // queue order feedback (rt_kernel.hip KArgs::tile_order): depths measured by the last frame of this tile geometry
  struct OrderKey {         // tile geometry (+ row tiles) an order belongs to: compared field by field
    uint32_t n_tiles = 0, tile_log2 = 0, tile_shape = 0, aff_group_log2 = 0, tile_rows = 0, first_tile = 0, tile_stride = 0, local_rows = 0;
    bool operator==(const OrderKey& o) const {
      return n_tiles == o.n_tiles && tile_log2 == o.tile_log2 && tile_shape == o.tile_shape && aff_group_log2 == o.aff_group_log2 &&
             tile_rows == o.tile_rows && first_tile == o.first_tile && tile_stride == o.tile_stride && local_rows == o.local_rows;
    }
  };
  struct Order {
    DevBuf tile_depth, tile_order;
    OrderKey key;             // n_tiles == 0: none yet
    bool ready = false;       // tile_order holds an order for key
    bool fresh = false;       // tile_depth holds depths of THIS view (measured by its last frame) that tile_order does not reflect yet
    int age = 0;              // frames since the order was last invalidated (geometry / camera / option change)
    void forget() { ready = false; fresh = false; age = 0; }  // (the buffers stay: the next frames measure into them)
  } order;
  DevBuf light_overflow;    // lit scenes: 560 B per lane of the largest launch so far (rt_core.h lane_light_begin)
  uint32_t last_pool_slots = 0, last_base_slots = 0; size_t last_lds_bytes = 0; bool last_lds_tables = false;  // of the last launch (rt_hip_scene_query)
  int last_kernel = -1;    // megakernel instantiation of the last launch, its Kernel::key (rt_hip_scene_query "last_kernel"; -1: none yet)

  // What rt_hip_wait reports about a launch lives in one of two SLOTS, used alternately: its event pair, the rows and waves
  // it covered, and a pinned host copy of its counters that an async copy fills right behind the kernel (stream-ordered:
  // the next launch's counter reset cannot overtake it).  Two launches of a scene may therefore be in flight on its stream
  // — frame i+1 rendering while frame i is gathered, rt_hip_group_submit / _collect — and a wait never issues a synchronous
  // device-to-host copy (it cost every rank of a multi-GPU frame ~25 us on the frame's critical path).
  struct Slot {
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_copied = nullptr;
    unsigned long long* h_counters = nullptr;  // pinned, RT_SLOT_COUNTERS words
    uint32_t rows = 0;
    uint64_t samples = 0;      // rows x width x samples per pixel AS LAUNCHED (an option set between submit and collect must not show)
    uint64_t waves = 0;
    bool launched = false;   // a kernel ran for it (false: an empty shard)
    std::chrono::steady_clock::time_point t_launch;
  } slot[2];
  uint64_t n_launches = 0;   // launch i uses slot[i & 1]
  hipStream_t last_stream = nullptr;
  bool in_flight = false;  // a launch has been enqueued and rt_hip_wait has not returned for it yet
  uint64_t last_waves = 0;
  uint32_t last_tiles_x = 0;
  // progressive rendering, host form (rt_hip_refine_to_host): the scene's own accumulator (width x height x 3 u64, allocated at
  // first use) and the samples per pixel it holds; zero: it must be cleared before the next pass adds to it.
  // ... denoised (rt_hip_refine_to_host_denoised): the resolved linear frame (x 12 B; the temporal form resolves into it too)
  // and the AOV record of the accumulator's start (x 32 B), allocated at first use.  aov_ready: dn_aov holds the AOVs of the current accumulator
  struct Progressive {
    DevBuf accum;
    uint32_t samples = 0;
    bool zero = true;
    DevBuf dn_lin, dn_aov;
    bool aov_ready = false;
    void reset() { samples = 0; zero = true; aov_ready = false; }
  } prog;
  DevBuf dn_ping;           // denoising (rt_hip_denoise): the filter's float4 ping-pong (2 x width x height x 16 B), allocated at first use
  // temporal denoising, host form (rt_hip_render_frame_temporal_to_host): the frame's own accumulator (x 24 B), and
  // two histories (x 16 B) and guide records (x 32 B) used alternately — cur names the pair the last frame wrote — with the
  // camera of that frame; all allocated at first use.  valid: the pair holds a frame.
  // ... with surface tracking (rt_hip_temporal_surface): two surface records (x 16 B) used alternately like the guides,
  // the displacement table (n_spheres x 24 B) and its host staging (kept as long as the scene: HIP copied from it), and each sphere's
  // centre at shutter time 0.5 of the tables the last temporal frame rendered with.  Allocated at first use in surface mode only.
  struct Temporal {
    DevBuf accum, hist[2], aov[2];
    int cur = 0;
    bool valid = false;
    double cam[12] = {};
    float k[5] = {RT_TEMPORAL_ALPHA_MIN, RT_TEMPORAL_N_MAX, RT_TEMPORAL_TAU_NORMAL, RT_TEMPORAL_TAU_ALBEDO, RT_TEMPORAL_TAU_INV_DEPTH};
    bool surface = false;
    float alpha_specular = RT_TEMPORAL_SURFACE_ALPHA_SPECULAR;
    DevBuf surf[2], disp;
    std::vector<double> mid, disp_host;
    // the history and every buffer go (freed on the current device; the caller has drained the stream that used them); what
    // rt_hip_temporal_configure and rt_hip_temporal_surface set stays, and so does the staging
    void reset() {
      Temporal none;
      std::memcpy(none.k, k, sizeof k); none.surface = surface; none.alpha_specular = alpha_specular;
      none.disp_host.swap(disp_host);
      *this = std::move(none);
    }
  } tp;
  // adaptive frames, host form (rt_hip_render_adaptive_to_host): its own now / prev accumulators and per-tile list, errors and
  // counts (allocated at first use), and what each round of the last frame did: {tiles, samples per pixel after it, kernel ms}
  struct Adaptive {
    DevBuf now, prev, list, err, spp;
    struct Round { uint32_t tiles, spp; double kernel_ms; };
    std::vector<Round> rounds;
    void reset() { rounds.clear(); }
  } ad;
  Slot& last_slot() { return slot[(n_launches + 1) & 1]; }  // the slot of the most recent launch
};
constexpr uint32_t RT_SLOT_COUNTERS = 32;  // segments, exact tests, tex_oob, grid steps, 4 x wave trip counts, 8 x section cycles, profile clocks, (the tile-queue cursors,) [28] repeated segments

extern "C" const char* rt_hip_last_error(void) { return g_err.c_str(); }

extern "C" uint32_t rt_abi_version(void) { return RT_ABI_VERSION; }
extern "C" size_t rt_abi_sizeof(const char* name) {
  if (!name) return 0;
  if (!std::strcmp(name, "RtSphere")) return sizeof(RtSphere);
  if (!std::strcmp(name, "RtQuad")) return sizeof(RtQuad);
  if (!std::strcmp(name, "RtTexture")) return sizeof(RtTexture);
  if (!std::strcmp(name, "RtScene")) return sizeof(RtScene);
  if (!std::strcmp(name, "RtRowTiles")) return sizeof(RtRowTiles);
  if (!std::strcmp(name, "RtStats")) return sizeof(RtStats);
  if (!std::strcmp(name, "RtGroupInfo")) return sizeof(RtGroupInfo);
  if (!std::strcmp(name, "RtGroupRank")) return sizeof(RtGroupRank);
  return 0;
}

extern "C" const char* rt_strerror(int code) {
  switch (code) {
    case RT_OK: return "ok";
    case RT_ERR_INVALID: return "invalid argument or inconsistent scene";
    case RT_ERR_NO_DEVICE: return "no gfx950 GPU visible (this library has no CPU fallback)";
    case RT_ERR_HIP: return "HIP runtime error";
    case RT_ERR_IO: return "Unable to read config file.";
    case RT_ERR_PARSE: return "Unable to parse config json";
    case RT_ERR_TEXTURE: return "failed to open/decode texture";
    case RT_ERR_PNG: return "error writing image";
    case RT_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown error";
  }
}

extern "C" int rt_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int rt_hip_device_warm(int device) {
  const int n = rt_hip_device_count();
  if (n <= 0) return fail(RT_ERR_NO_DEVICE, rt_strerror(RT_ERR_NO_DEVICE));
  if (device < 0 || device >= n) return fail(RT_ERR_INVALID, "device index out of range");
  RT_HIP_TRY(hipSetDevice(device));
  void* p = nullptr;
  RT_HIP_TRY(hipMalloc(&p, 256));  // (the first allocation creates the device's context)
  hipLaunchKernelGGL(rtk::rt_warm_up, dim3(1), dim3(64), 0, nullptr);  // (the first launch loads this library's code object)
  RT_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rtk::rt_warm_up_scratch, dim3(1), dim3(64), 0, nullptr, (uint32_t*)nullptr, 1u);  // (... and gives the NULL stream's queue its scratch memory)
  RT_HIP_TRY(hipGetLastError());
  RT_HIP_TRY(hipDeviceSynchronize());
  (void)hipFree(p);
  return RT_OK;
}

extern "C" void rt_hip_scene_destroy(RtHipScene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (auto& sl : s->slot) {
    for (hipEvent_t e : {sl.ev_start, sl.ev_stop, sl.ev_copied}) if (e) (void)hipEventDestroy(e);
    if (sl.h_counters) (void)hipHostFree(sl.h_counters);
  }
  delete s;
}

namespace {
int room(DevBuf& b, size_t bytes) { return b.ensure(bytes ? bytes : 16); }  // (an empty table is 16 bytes, never a null pointer)
template <typename V>
int upload(DevBuf& dst, const V& v) {
  const size_t bytes = v.size() * sizeof(typename V::value_type);
  const int rc = room(dst, bytes);
  if (rc != RT_OK) return rc;
  if (bytes) RT_HIP_TRY(hipMemcpy(dst.p, v.data(), bytes, hipMemcpyHostToDevice));
  return RT_OK;
}
// the structure just built (creation and every rebuild) into generation `g`, and what a refit needs of it: derived on the host from the static
// topology, uploaded once
int upload_flat_structure(RtHipScene::Resident::Flats& f, RtHipScene::Resident::Flats::Tables& g, const std::vector<rtc::FlatNode>& nodes,
                          const std::vector<uint32_t>& order, uint32_t n_always) {
  int rc;
  if ((rc = upload(g.nodes, nodes)) != RT_OK || (rc = upload(g.order, order)) != RT_OK) return rc;
  rtc::flat_topology(nodes, order, n_always, f.topo);
  f.start_ready = false;
  if ((rc = upload(f.boxed, f.topo.boxed)) != RT_OK || (rc = upload(f.leaves, f.topo.leaves)) != RT_OK) return rc;
  return upload(f.levels, f.topo.level_nodes);
}
// before a scene or a view takes other tables: its device is current, and a launch in flight has finished (its stream is synchronised)
int make_current_and_drain(RtHipScene* s) {
  RT_HIP_TRY(hipSetDevice(s->device));
  if (s->n_launches && s->in_flight) { RT_HIP_TRY(hipStreamSynchronize(s->last_stream)); s->in_flight = false; }
  return RT_OK;
}
}  // namespace

namespace {
// what a LAUNCH of a scene writes: the counter block with the tile-queue cursors, the two stats slots (events + pinned words)
int alloc_launch_state(RtHipScene* s) {
  const size_t counter_bytes = (32 + 4 * RT_TIMELINE_WAVES) * sizeof(unsigned long long);
  const int rc = s->counters.ensure(counter_bytes);
  if (rc != RT_OK) return rc;
  for (auto& sl : s->slot) {
    if (hipEventCreate(&sl.ev_start) != hipSuccess || hipEventCreate(&sl.ev_stop) != hipSuccess ||
        hipEventCreateWithFlags(&sl.ev_copied, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void**)&sl.h_counters, RT_SLOT_COUNTERS * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
      return fail(RT_ERR_HIP, "hipEventCreate/hipHostMalloc failed");
    std::memset(sl.h_counters, 0, RT_SLOT_COUNTERS * sizeof(unsigned long long));
  }
  if (hipMemset(s->counters.p, 0, counter_bytes) != hipSuccess)
    return fail(RT_ERR_HIP, "hipMemset failed");
  return RT_OK;
}
}  // namespace

// A second VIEW of a resident scene (internal; the group's overlapped frames): the same tables and textures in HBM, its own
// launch state — so that a launch of the view and a launch of the scene may be in flight on two streams AT ONCE (a scene itself
// is not re-entrant: one tile-queue cursor, one counter block).  The scene and its views may be destroyed in any order.
int rt_hip_scene_clone_view(const RtHipScene* src, RtHipScene** out) {
  if (!src || !out) return fail(RT_ERR_INVALID, "null argument");
  *out = nullptr;
  RT_HIP_TRY(hipSetDevice(src->device));
  RtHipScene* s = new RtHipScene;
  s->device = src->device; s->res = src->res; s->host = src->host; s->dev = src->dev; s->opt = src->opt;
  int rc = alloc_launch_state(s);
  if (rc == RT_OK) rc = warm_up(s);  // (the launch configuration + the lit kernels' overflow slots, outside any frame)
  if (rc == RT_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(RT_ERR_HIP, "hipDeviceSynchronize failed");
  if (rc != RT_OK) { rt_hip_scene_destroy(s); return rc; }
  *out = s;
  return RT_OK;
}

extern "C" int rt_hip_scene_create(const RtScene* scene, int device, RtHipScene** out) {
  return rt_hip_scene_create_moving(scene, nullptr, device, out);
}

// motion blur: the tables of a scene whose spheres move from center to center1 over the shutter.  Fixed at creation
// (the grid lists each moving sphere by its swept box); a null center1, or one equal to every centre, is the static scene.
extern "C" int rt_hip_scene_create_moving(const RtScene* scene, const double* center1, int device, RtHipScene** out) {
  return rt_hip_scene_create_quads(scene, center1, nullptr, 0, device, out);
}

// quads: the scene above plus n_quads flat parallelograms, tested behind the spheres by the QUADS kernels; without a quad every
// table and every kernel is what rt_hip_scene_create_moving always built and selected
namespace { int scene_create_flats(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, int device, RtHipScene** out, bool flat_bvh); }
extern "C" int rt_hip_scene_create_quads(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, int device, RtHipScene** out) {
  return scene_create_flats(scene, center1, quads, n_quads, device, out, false);
}
// the structure: the scene above with a BVH over its flat primitives, which lifts their cap to RT_MAX_FLATS_BVH.  The count
// is checked before any record is read, and there must be a flat primitive to build over.
extern "C" int rt_hip_scene_create_flats_bvh(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, int device, RtHipScene** out) {
  if (out) *out = nullptr;
  if (n_quads > RT_MAX_FLATS_BVH) return fail(RT_ERR_UNSUPPORTED, "more than RT_MAX_FLATS_BVH (2^20) flat primitives");
  if (n_quads == 0) return fail(RT_ERR_INVALID, "a flat BVH needs at least one flat primitive");
  return scene_create_flats(scene, center1, quads, n_quads, device, out, true);
}
namespace {
int scene_create_flats(const RtScene* scene, const double* center1, const RtQuad* quads, uint32_t n_quads, int device, RtHipScene** out, bool flat_bvh) {
  if (!scene || !out || (n_quads && !quads)) return fail(RT_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!flat_bvh && n_quads > RT_MAX_QUADS) return fail(RT_ERR_UNSUPPORTED, "more than RT_MAX_QUADS (1024) quads: every segment tests every quad");
  int n = rt_hip_device_count();
  if (n <= 0) return fail(RT_ERR_NO_DEVICE, rt_strerror(RT_ERR_NO_DEVICE));
  if (device < 0 || device >= n) return fail(RT_ERR_INVALID, "device index out of range");
  rtp::Clock pc = rtp::begin();
  rtc::HostTables t;
  std::string why = rtc::build_tables(*scene, t, false, center1, quads, n_quads);
  if (!why.empty()) return fail(RT_ERR_INVALID, why);
  if (const int refused = check_wide_tables(t.grid.wide, t.n_media, t.n_solids, n_quads != 0)) return refused;
  if (flat_bvh) {
    why = rtc::build_flat_bvh(t);
    if (!why.empty()) return fail(RT_ERR_INVALID, why);
  }
  pc.mark("scene.tables_and_grid");
  rtc::build_texels(*scene, t);
  pc.mark("scene.texels_rgbx");
  RT_HIP_TRY(hipSetDevice(device));
  auto r = std::make_shared<RtHipScene::Resident>();
  r->device = device;
  r->has_lights = !t.lights.empty();
  r->sphere_lights = t.lights;
  if (n_quads) {  // (§28: what rt_hip_scene_set_flat_lights puts back when an entry stops emitting)
    r->keep_flat_mat.assign(t.mat.begin() + scene->n_spheres, t.mat.end());
    r->keep_flat_matc.assign(t.matc.begin() + scene->n_spheres, t.matc.end());
  }
  r->simple_colour = t.simple_colour;
  RtHipScene::Resident::Spheres::Tables& live = r->sph.live;
  RtHipScene::Resident::Flats& f = r->flat;
  live.grid = t.grid;
  r->sph.spheres.assign(scene->spheres, scene->spheres + scene->n_spheres);
  r->sph.set_mid(t.motion);
  {
    hipDeviceProp_t prop;
    RT_HIP_TRY(hipGetDeviceProperties(&prop, device));
    r->num_cus = prop.multiProcessorCount;
    // 160 KB of LDS per CU on gfx950; the unlit layouts stay below LDS_TABLES_MAX_BYTES (156 KB) as before, the light pools may
    // take what the device says is left
    const size_t dev_lds = prop.sharedMemPerBlock > prop.maxSharedMemoryPerMultiProcessor ? prop.sharedMemPerBlock : prop.maxSharedMemoryPerMultiProcessor;
    r->lds_cap = std::max<size_t>(rtk::LDS_TABLES_MAX_BYTES, std::min<size_t>(dev_lds, 160u * 1024u));
  }
  pc.mark("scene.device_properties");
  int rc;
  if ((rc = upload(live.geom, t.geom)) != RT_OK) return rc;
  if ((rc = upload(r->mat, t.mat)) != RT_OK) return rc;
  if ((rc = upload(r->lights, t.lights)) != RT_OK) return rc;
  if ((rc = upload(r->matc, t.matc)) != RT_OK) return rc;
  if ((rc = upload(live.cell_word, t.cell_word)) != RT_OK) return rc;
  if ((rc = t.grid.wide ? upload(live.cell_items, t.cell_items32) : upload(live.cell_items, t.cell_items)) != RT_OK) return rc;  // (wide tables: the 32-bit item lists)
  if ((rc = upload(live.large, t.large)) != RT_OK) return rc;
  if ((rc = upload(live.large_geom, t.large_geom)) != RT_OK) return rc;
  if (t.n_moving && (rc = upload(live.motion, t.motion)) != RT_OK) return rc;
  live.n_moving = t.n_moving;
  if (t.n_media && (rc = upload(r->medium, t.medium)) != RT_OK) return rc;
  r->n_media = t.n_media;
  r->n_solids = t.n_solids;
  f.n_quads = n_quads;
  if (!t.quad_lim.empty() && (rc = upload(f.lim, t.quad_lim)) != RT_OK) return rc;
  f.n_tris = t.n_tris;
  f.n_nodes = (uint32_t)t.flat_nodes.size(); f.host_lim = t.quad_lim;
  if (flat_bvh) {  // (§22: the records behind their header, one buffer; the header holds the device addresses of the four tables)
    if ((rc = upload_flat_structure(f, f.live, t.flat_nodes, t.flat_order, t.flat_always)) != RT_OK) return rc;
    if ((rc = f.live.rec.ensure(t.flat_blob.size() * sizeof(RtQuadRec))) != RT_OK) return rc;
    const rtc::FlatBvhHeader h = f.header(f.state(), f.first_rec(f.live), scene->n_spheres);
    std::memcpy(t.flat_blob.data(), &h, sizeof h);
    RT_HIP_TRY(hipMemcpy(f.live.rec.p, t.flat_blob.data(), t.flat_blob.size() * sizeof(RtQuadRec), hipMemcpyHostToDevice));
  } else if (n_quads && (rc = upload(f.live.rec, t.quads)) != RT_OK) return rc;
  {
    std::vector<uint32_t> all(scene->n_spheres);
    for (uint32_t i = 0; i < scene->n_spheres; ++i) all[i] = i;
    if ((rc = upload(r->sph.all, all)) != RT_OK) return rc;
  }
  pc.mark("scene.upload_tables");
  // textures and sky: resident as 4-byte texels (rt_tables.h build_texels; one dword load per fetch); the caller's RGB8
  // bytes are uploaded too only if some record is outside that path's range (rt_core.h texels_fast)
  r->texel_bytes = (t.tex4.size() + t.sky4.size()) * 4u;
  if ((rc = upload(r->tex4, t.tex4)) != RT_OK) return rc;
  if ((rc = upload(r->sky4, t.sky4)) != RT_OK) return rc;
  {
    std::vector<uint8_t>& blob = r->keep_tex_rgb8;
    blob.assign(t.need_rgb8 ? t.tex_bytes : 0, 0);
    if (t.need_rgb8)
      for (uint32_t i = 0; i < scene->n_textures; ++i)
        if (scene->textures[i].nbytes) std::memcpy(&blob[t.tex_off[i]], scene->textures[i].rgb8, scene->textures[i].nbytes);
    if ((rc = upload(r->tex, blob)) != RT_OK) return rc;
  }
  {
    std::vector<uint8_t>& sky = r->keep_sky_rgb8;
    if (scene->sky_mode == RT_SKY_TEXTURE && !t.sky_fast) sky.assign(scene->sky_rgb8, scene->sky_rgb8 + scene->sky_w * scene->sky_h * 3);
    if ((rc = upload(r->sky, sky)) != RT_OK) return rc;
  }
  r->keep_tex4.swap(t.tex4); r->keep_sky4.swap(t.sky4);
  if (n_quads && scene->n_textures) {  // (§29: what rt_hip_scene_set_flat_images' prepare kernel knows of the textures; build_texels' layout)
    std::vector<RtFlatImageTex> table(scene->n_textures);
    uint64_t before = 0;
    for (uint32_t i = 0; i < scene->n_textures; ++i) {
      const RtTexture& x = scene->textures[i];
      table[i] = rt_flat_image_tex(x.width, x.height, x.nbytes, before);
      // (the first texture that does not fit ends the expanded run: every later one is outside too)
      before = (table[i].ok == RT_FLAT_IMAGE_TEX_FAR || before + x.nbytes / 3 >= (1ull << 31)) ? (1ull << 31) : before + x.nbytes / 3;
    }
    if ((rc = upload(f.tex_table, table)) != RT_OK) return rc;
    f.n_textures = scene->n_textures;
  }
  f.tex4_dev = r->tex4.get<const uint32_t>();
  pc.mark("scene.upload_texels");
  RtHipScene* s = new RtHipScene;
  s->device = device;
  s->host = *scene;
  s->host.spheres = nullptr; s->host.textures = nullptr; s->host.sky_rgb8 = nullptr;
  rtc::fill_dev_scene(*scene, t, s->dev);
  r->point(s->dev);
  s->res = std::move(r);
  auto bail = [&](int code) { rt_hip_scene_destroy(s); return code; };
  if ((rc = alloc_launch_state(s)) != RT_OK) return bail(rc);
  // Everything above went through the NULL stream — and hipMemset / hipMemcpy from pageable memory return before the device
  // has finished (they are asynchronous to the host: the fill / the DMA out of the staging buffer may still be queued).
  // The frames run on the CALLER's streams, and a non-blocking stream does not order itself behind the NULL stream: a first
  // frame launched right away could start before the tables had landed, or have its tile-queue cursor zeroed under it
  // (round 4: the group launches rank 0 from the creating thread at once — 65 % of fresh 3-rank groups traced tiles twice).
  // ... and nothing a first frame should pay for is left for it: the code object on the device, the default configuration's
  // kernel attribute / occupancy / (lit scenes) overflow slots (a one-shot rt_render_rgb8 — the reference renders one frame per
  // process — reports this under setup_ms, outside its frame_ms window)
  pc.mark("scene.counters_events_pinned_words");
  if ((rc = warm_up(s)) != RT_OK) return bail(rc);
  pc.mark("scene.kernel_configuration");
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(RT_ERR_HIP, "hipDeviceSynchronize failed"));
  pc.mark("scene.device_idle");
  *out = s;
  return RT_OK;
}
}  // namespace

extern "C" int rt_hip_set_option(RtHipScene* s, const char* key, int64_t value) {
  if (!s || !key) return fail(RT_ERR_INVALID, "null argument");
  constexpr int64_t max_variant = 1;
  if (!std::strcmp(key, "variant")) { if (value < 0 || value > max_variant) return fail(RT_ERR_INVALID, "variant must be 0 (grid walk) or 1 (brute force)"); s->opt.variant = (int)value; return RT_OK; }
  if (!std::strcmp(key, "tile_log2")) { if (value < -1 || value > 3) return fail(RT_ERR_INVALID, "tile_log2 must be -1..3"); s->opt.tile_log2 = (int)value; return RT_OK; }
  if (!std::strcmp(key, "tile_shape")) { if (value < 0 || value > 3) return fail(RT_ERR_INVALID, "tile_shape must be 0 (square), 1 (scanline runs), 2 (4:1) or 3 (16:1)"); s->opt.tile_shape = (int)value; return RT_OK; }
  if (!std::strcmp(key, "tile_affinity")) { if (value < 0 || value > 2) return fail(RT_ERR_INVALID, "tile_affinity must be 0 (off), 1 (large frames) or 2 (any frame of 8+ runs: tests)"); s->opt.tile_affinity = (int)value; s->order.forget(); return RT_OK; }
  if (!std::strcmp(key, "tile_order")) { if (value < 0 || value > 2) return fail(RT_ERR_INVALID, "tile_order must be 0, 1 or 2"); s->opt.order_mode = (int)value; s->order.forget(); return RT_OK; }
  if (!std::strcmp(key, "light_pool")) { if (value < 0 || value > 1024 || (value != 0 && value < 32)) return fail(RT_ERR_INVALID, "light_pool must be 0 (automatic) or 32..1024"); s->opt.light_pool_cap = (int)value; return RT_OK; }
  if (!std::strcmp(key, "light_base_pool")) { if (value < 0 || value > 1024 || (value != 0 && value < 32)) return fail(RT_ERR_INVALID, "light_base_pool must be 0 (automatic) or 32..1024"); s->opt.light_base_cap = (int)value; return RT_OK; }
  if (!std::strcmp(key, "light_nest_pool")) { if (value < 0 || value > 1) return fail(RT_ERR_INVALID, "light_nest_pool must be 0 or 1"); s->opt.light_nest_pool = (int)value; return RT_OK; }
  if (!std::strcmp(key, "force_lit")) { if (value < 0 || value > 1) return fail(RT_ERR_INVALID, "force_lit must be 0 or 1"); s->opt.force_lit = (int)value; return RT_OK; }  // (diagnostics: an unlit scene through the lit kernels — what their code costs the ordinary lanes, profiles/r04_run5_lit_sections.log)
  if (!std::strcmp(key, "tile_batch")) { if (value < 0 || value > 64) return fail(RT_ERR_INVALID, "tile_batch must be 0..64"); s->opt.tile_batch = (int)value; return RT_OK; }
  if (!std::strcmp(key, "flat_build")) { if (value < 0 || value > 1) return fail(RT_ERR_INVALID, "flat_build must be 0 (the host builds) or 1 (the device builds)"); s->opt.flat_build = (int)value; return RT_OK; }
  if (!std::strcmp(key, "chunk_spp")) { if (value < 0) return fail(RT_ERR_INVALID, "chunk_spp must be >= 0"); s->opt.chunk_spp = (int)value; return RT_OK; }
  if (!std::strcmp(key, "samples_per_pixel") || !std::strcmp(key, "max_depth")) {
    if (value < 0 || value > (int64_t)0xFFFFFFFFll) return fail(RT_ERR_INVALID, std::string(key) + " must be in 0 .. 2^32-1");
    if (key[0] == 's') s->host.samples_per_pixel = s->dev.spp = (uint32_t)value;
    else { s->host.max_depth = s->dev.max_depth = (uint32_t)value; s->prog.reset(); }
    return RT_OK;
  }
  if (!std::strcmp(key, "seed")) { s->host.seed = (uint64_t)value; s->dev.seed_lo = (uint32_t)value; s->dev.seed_hi = (uint32_t)((uint64_t)value >> 32); s->prog.reset(); return RT_OK; }
  if (!std::strcmp(key, "accum_reset")) { if (value != 1) return fail(RT_ERR_INVALID, "accum_reset takes the value 1"); s->prog.reset(); return RT_OK; }
  return fail(RT_ERR_INVALID, std::string("unknown option ") + key);
}

namespace {

// The megakernel instantiations by key (rt_kernel.hip): set 0, which this unit always compiles, and the slices of the sets 1 - 7 side by
// side.  A null entry is a key that is not valid.
using rtk::Megakernel;
template <int... SET> std::array<Megakernel, rtk::KERNEL_KEYS> kernel_table(std::integer_sequence<int, SET...>) {
  const rtk::KernelSetTable sets[] = {rtk::kernel_set_table<0>(std::make_integer_sequence<int, rtk::KERNEL_SET_KEYS>()), rtk::kernel_set<SET + 1>()...};
  std::array<Megakernel, rtk::KERNEL_KEYS> t;
  for (int key = 0; key < rtk::KERNEL_KEYS; ++key) {
    t[key] = sets[key / rtk::KERNEL_SET_KEYS][key % rtk::KERNEL_SET_KEYS];
    if ((t[key] != nullptr) != rtk::kernel_key_valid(key)) std::abort();  // (holds while megakernel_of_key decides by this predicate: the table cannot drift from it unnoticed)
  }
  return t;
}
struct Kernel { int key = -1; Megakernel fn = nullptr; };
int select_kernel(const RtHipScene* s, bool has_lights, bool lds_tables, bool wide, bool accum, Kernel* out) {
  static const std::array<Megakernel, rtk::KERNEL_KEYS> table = kernel_table(std::make_integer_sequence<int, rtk::KERNEL_SETS - 1>());
  const int key = (s->res->flat.n_quads ? rtk::KEY_QUADS : 0) | (s->res->n_solids ? rtk::KEY_SOLID : 0) | (s->dev.medium ? rtk::KEY_MEDIUM : 0) | (s->dev.motion ? rtk::KEY_MOTION : 0) |
                  (s->dev.lens_r != 0.0 ? rtk::KEY_LENS : 0) | (accum ? rtk::KEY_ACCUM : 0) | (wide ? rtk::KEY_WIDE : 0) | (has_lights ? rtk::KEY_HL : 0) |
                  (s->res->simple_colour ? rtk::KEY_SIMPLE : 0) | (lds_tables ? rtk::KEY_LDS : 0);
  if (!rtk::kernel_key_valid(key)) {
    if (key & rtk::KEY_LDS) return fail(RT_ERR_HIP, "wide cell tables cannot be staged in LDS");
    if ((key & rtk::KEY_QUADS) && !(key & rtk::KEY_WIDE)) return fail(RT_ERR_HIP, "the QUADS kernels take their tables from L2 and the general colour map");
    if (key & rtk::KEY_MEDIUM) return fail(RT_ERR_UNSUPPORTED, "participating media with wide tables");
    if (key & rtk::KEY_SOLID) return fail(RT_ERR_UNSUPPORTED, "solid textures with wide tables");
    return fail(RT_ERR_UNSUPPORTED, "quads with wide tables");
  }
  out->key = key;
  out->fn = table[key];
  return RT_OK;
}

// Everything a launch needs that is NOT the launch: the kernel's dynamic-LDS attribute and its occupancy (worked out once per
// configuration: two runtime calls a frame otherwise) and, lit kernels, the lanes' HBM overflow slots.  Runs BEFORE the
// launch's start event is recorded — a first frame used to carry the 147 MB hipMalloc of a lit scene and the runtime's
// first look at the kernel inside its kernel_ms (one-shot CLI frames: 8.4 ms for a 0.9 ms kernel, profiles/r05_run5_cli_stats_before_warmup.log)
// — and once at scene creation for the scene's default configuration (warm_up).
int prepare(RtHipScene* s, const Kernel& k, size_t lds_bytes, hipStream_t stream) {
  if (s->cfg_key != k.key || s->cfg_lds != lds_bytes) {
    if (lds_bytes > 48 * 1024) RT_HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int per_cu_q = 0;
    RT_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_q, k.fn, rtk::BLOCK, lds_bytes));
    if (per_cu_q < 1) return fail(RT_ERR_HIP, "megakernel does not fit on a CU");
    s->cfg_key = k.key; s->cfg_lds = lds_bytes; s->cfg_per_cu = per_cu_q;
  }
  if (k.key & 4) {  // the lanes' overflow slots for suspended light activations (rt_core.h lane_light_begin): for the resident set, kept
    // (an earlier launch of this scene may still be running on this stream with the old buffer: it drains that stream first — once
    //  per scene and configuration, never in a frame loop)
    const size_t need_bytes = (size_t)s->cfg_per_cu * (size_t)s->res->num_cus * rtk::BLOCK * rtc::LIGHT_OVERFLOW_BYTES_PER_LANE;
    return s->light_overflow.ensure(need_bytes, nullptr, stream);
  }
  return RT_OK;
}
void launch(RtHipScene* s, const Kernel& k, rtk::KArgs ka, size_t lds_bytes, uint32_t n_items, hipStream_t stream) {
  s->last_kernel = k.key;  // (here, not in prepare: warm_up prepares the scene's default configuration without launching it)
  // persistent: exactly the resident set, never more workgroups than there are wave-sized items
  uint32_t wgs = (uint32_t)s->cfg_per_cu * (uint32_t)s->res->num_cus;
  const uint32_t need = (n_items + rtk::WAVES - 1) / rtk::WAVES;
  if (wgs > need) wgs = need;
  s->last_waves = (uint64_t)wgs * rtk::WAVES;
  if (k.key & 4) ka.sc.light_overflow = s->light_overflow.get<unsigned char>();
  hipLaunchKernelGGL(k.fn, dim3(wgs), dim3(rtk::BLOCK), lds_bytes, stream, ka);
}

// LDS budget of a launch: do the tables fit, how big are the light pools, how much dynamic LDS does a workgroup ask for.
struct LdsPlan { bool lds_tables = false; uint32_t pool_slots = 0, base_slots = 0; size_t lds_bytes = 0; };
// n_lights: the light count the pools are sized for (-1: the scene's own)
int plan_lds(const RtHipScene* s, const rtc::GridDesc& G, bool has_lights, LdsPlan* out, int64_t n_lights = -1) {
  // LDS budget.  Tables + tile slots + (lit scenes) the two pools of light records (rt_core.h): frames — held by a lane while
  // it sums over the lights — and, with the short colour map, bases — held from a sample's first light sampling to its end.
  // Expected demand: a camera path starts summing over the n lights with probability ~0.1 n at each of its first two hits
  // (raytracer.rs:92-102) and then shoots n light rays, so about f = 0.2 n^2 / (2.9 + 0.2 n^2) of the lanes hold a frame at
  // any moment (n = 1: 6.5 % = 66 of 1024 lanes; n = 2: 22 %; n = 3: 38 %) and about b = 0.2 n (n + 2) / (2.9 + 0.2 n^2) a
  // base (n = 1: 19 %).  A lane that finds a pool exhausted repeats its segment, so undersized pools are slow, never wrong
  // (forced pools of 64 / 32 frames on the lit cover scene: +1 % / +64 %, profiles/r03_run*_lit.log).  The pools get what is
  // left beside the tables, in the proportion of their demands, up to one record per lane; if that is less than 1.2 x the
  // demand the TABLES stay in L2 instead and the pools take their room.
  const bool short_map = has_lights && s->res->simple_colour;
  uint32_t pool_slots = 0, base_slots = 0;
  auto size_pools = [&](size_t avail, double* margin) {  // largest x with frames = x f 1024, bases = x b 1024 (multiples of 32, 32 .. 1024) inside `avail`
    const double n = (double)(n_lights < 0 ? s->dev.n_lights : (uint32_t)n_lights), den = 2.9 + 0.2 * n * n;
    const double f = std::max(0.2 * n * n / den, 1.0 / 64.0), b = short_map ? std::min(1.0, std::max(0.2 * n * (n + 2.0) / den, 1.0 / 64.0)) : 0.0;
    auto slots = [&](double x, double share) -> uint32_t {
      if (share == 0.0) return 0u;
      const double v = x * share * (double)rtk::BLOCK;
      const uint32_t q = v >= (double)rtc::LIGHT_POOL_MAX_SLOTS ? rtc::LIGHT_POOL_MAX_SLOTS : ((uint32_t)v & ~31u);
      return q < 32u ? 32u : q;
    };
    auto bytes = [&](double x) { return (size_t)((rtk::park_bytes(slots(x, f), slots(x, b)) + 15u) & ~15u); };
    double lo = 0.0, hi = 1.0 / std::min(f, b > 0.0 ? b : f) + 1.0;  // at `hi` both pools hold one record per lane
    if (bytes(hi) <= avail) lo = hi;
    else for (int it = 0; it < 40; ++it) { const double mid = 0.5 * (lo + hi); if (bytes(mid) <= avail) lo = mid; else hi = mid; }
    pool_slots = slots(lo, f); base_slots = slots(lo, b);
    const bool forced_f = s->opt.light_pool_cap > 0, forced_b = s->opt.light_base_cap > 0;  // (tests: small pools on purpose)
    if (forced_f && pool_slots > (uint32_t)s->opt.light_pool_cap) pool_slots = (uint32_t)s->opt.light_pool_cap & ~31u;
    if (forced_b && base_slots > (uint32_t)s->opt.light_base_cap) base_slots = (uint32_t)s->opt.light_base_cap & ~31u;
    if (margin) *margin = (forced_f || forced_b) ? 1e9 : std::min((double)pool_slots / (f * rtk::BLOCK), b > 0.0 ? (double)base_slots / (b * rtk::BLOCK) : 1e9);
    return bytes(0.0) <= avail;  // (the smallest pools fit)
  };
  const rtk::LdsLayout no_pools = rtk::lds_layout(s->host.n_spheres, G.n_cells, G.n_items, true, false);
  bool lds_tables = !G.wide && !s->res->flat.n_quads && no_pools.total <= rtk::LDS_TABLES_MAX_BYTES;  // (the QUADS kernels exist with tables in L2 only)
  if (has_lights) {
    const size_t fixed = rtc::LIGHT_CENTRES_LDS_MAX * 24u;
    double margin = 0.0;
    bool ok = lds_tables && no_pools.total + fixed < s->res->lds_cap && size_pools(s->res->lds_cap - no_pools.total - fixed, &margin) && margin >= 1.2;
    if (!ok) {
      lds_tables = false;
      const size_t bare = rtk::lds_layout(0, 0, 0, false, false).total + fixed;
      if (!size_pools(s->res->lds_cap - bare, nullptr)) return fail(RT_ERR_UNSUPPORTED, "no room for the light pools in LDS");
    }
  }
  out->lds_tables = lds_tables; out->pool_slots = pool_slots; out->base_slots = base_slots;
  out->lds_bytes = lds_tables ? rtk::lds_layout(s->host.n_spheres, G.n_cells, G.n_items, true, has_lights, pool_slots, base_slots).total
                              : rtk::lds_layout(0, 0, 0, false, has_lights, pool_slots, base_slots).total;
  return RT_OK;
}

// the launch configuration of the scene's tables and options: the LDS-or-L2 staging choice, the kernel, its attribute and occupancy
int configure(RtHipScene* s) {
  LdsPlan plan;
  int rc = plan_lds(s, s->dev.grid, s->res->has_lights, &plan);
  if (rc != RT_OK) return rc;
  Kernel k;
  if ((rc = select_kernel(s, s->res->has_lights, plan.lds_tables, s->dev.grid.wide != 0u, false, &k)) != RT_OK) return rc;
  return prepare(s, k, plan.lds_bytes, nullptr);
}
int warm_up(RtHipScene* s) {
  // (keeping every CU busy for 0.5 - 20 ms here does NOT make a first frame faster — it is not the clocks:
  //  profiles/r05_run7_cli_warm_spin.log)
  hipLaunchKernelGGL(rtk::rt_warm_up, dim3(1), dim3(64), 0, nullptr);
  RT_HIP_TRY(hipGetLastError());
  return configure(s);
}

}  // namespace

namespace {
// The pixel tiles of a launch over local_rows packed rows: the unit of the megakernel's queue, of list launches, of the adaptive
// frame's sample counts (rt_hip_tile_grid) and of rt_tile_error.  Tile id = ty * tiles_x + tx.
struct TileGeom { uint32_t tile_log2 = 0, tile_wl = 0, tile_hl = 0, tiles_x = 0, tiles_y = 0; };
int tile_geometry(const RtHipScene* s, uint32_t local_rows, TileGeom* out) {
  // Pixel tile: the unit of the global queue, owned by ONE workgroup.  8x8 when the frame has
  // >= ~100 tiles per workgroup; small frames (and the 1/8 shards of the multi-GPU run) use 4x4,
  // 2x2 or 1x1 tiles, so that the heaviest tile (glass: 10x the mean) is a small part of a
  // workgroup's share and the long-path regions spread over many workgroups.
  const uint64_t want_tiles = (uint64_t)s->res->num_cus * 100u;
  // tile geometry: 4^tl pixels, as a square (default) or a run of one scanline
  // (shape 0: 2^t x 2^t; 1: 4^t x 1; 2 and 3: the square widened / flattened once or twice, 16x4 and 32x2 at t = 3)
  // (default shape: squares — but the 2x2 tiles of a small frame / a multi-GPU shard as 4x1 strips: 12 contiguous bytes
  //  leave in one packed store instead of two rows of byte stores; same time, WRITE_SIZE 2.71 -> 2.17 MB on an 1/8 shard
  //  of the headline frame, profiles/r03_run10_shape_traffic_sweep.log)
  // (shape 2 at t = 1 is the 2x2 square — the A/B arm of the 4x1 default, which no other value selects)
  const int shape = s->opt.tile_shape;
  auto widen = [&](uint32_t t) { const uint32_t k = shape == 0 ? (t == 1u ? 1u : 0u) : (shape == 1 ? t : (shape == 2 && t == 1u ? 0u : (uint32_t)shape - 1u)); return k < t ? k : t; };
  auto tiles_xy = [&](uint32_t t, uint32_t& tx, uint32_t& ty) {
    const uint32_t wl = t + widen(t), hl = t - widen(t);
    tx = (s->host.width + (1u << wl) - 1) >> wl; ty = (local_rows + (1u << hl) - 1) >> hl;
  };
  uint32_t tl = s->opt.tile_log2 < 0 ? 3u : (uint32_t)s->opt.tile_log2, tx = 0, ty = 0;
  if (s->opt.tile_log2 < 0) {
    for (;;) { tiles_xy(tl, tx, ty); if (tl == 0 || (uint64_t)tx * ty >= want_tiles) break; tl--; }
  }
  // a slot header packs (tile column | tile row << 16), and the queue cursor is 32 bits
  auto too_many = [&](uint32_t t) { tiles_xy(t, tx, ty); return tx > 65535u || ty > 65535u || (uint64_t)tx * ty >= (1ull << 31); };
  while (tl < 3 && too_many(tl)) tl++;
  if (too_many(tl)) return fail(RT_ERR_UNSUPPORTED, "frame too large for the tile queue (more than 65535 tiles on an axis or 2^31 tiles)");
  out->tile_log2 = tl; out->tile_wl = tl + widen(tl); out->tile_hl = tl - widen(tl);
  out->tiles_x = tx; out->tiles_y = ty;
  return RT_OK;
}
}  // namespace

namespace {
// One launch of the megakernel over the given row tiles: samples [sample_base, sample_base + spp) of every pixel.  accum == nullptr:
// the one-shot frame (rt_hip_render: sample_base 0, the scene's samples per pixel, pixels into d_rgb8 / d_linear); else the
// accumulating kernels add the pass's sums to accum (rt_hip_accumulate).  list != nullptr (accumulating only): just the n_list
#ifdef RT_TEST_PROBES
// the camera rays and first-hit record of the launch rt_hip_render_rays_probe is making (KArgs.probe_rays); null otherwise
struct ProbeRays { const double* rays = nullptr; double* t = nullptr; int32_t* best = nullptr; };
ProbeRays g_probe_rays;
#endif
// tiles it names, in its order (rt_hip_accumulate_tiles); such a launch neither reads nor changes the scene's learned queue order,
// and `samples` counts n_list whole tiles.  The caller has checked its own arguments.
int launch_frame(RtHipScene* s, const RtRowTiles* tiles, void* d_rgb8, void* d_linear, unsigned long long* accum, uint32_t sample_base,
                 uint32_t spp, void* stream_, const uint32_t* list = nullptr, uint32_t n_list = 0) {
  const uint32_t local_rows = rt_tiles_local_rows(s->host.height, tiles);
  hipStream_t stream = (hipStream_t)stream_;
  const bool has_lights = s->res->has_lights || s->opt.force_lit != 0;
  // one tile-queue cursor / counter block per scene: launches of a scene are ordered on ONE stream
  // (a caller that drained the first stream itself — hipStreamSynchronize, an event — need not call rt_hip_wait first:
  //  the scene asks its OWN event, recorded behind the last launch's counter copy — never the caller's stream handle,
  //  which may have been destroyed since.  The abandoned launch's counters stay readable in its slot until two more
  //  launches have reused it; nobody waited for them.)
  if (s->in_flight && stream != s->last_stream && hipEventQuery(s->last_slot().ev_copied) != hipErrorNotReady) s->in_flight = false;
  (void)hipGetLastError();  // (the query's status is not an error of this call)
  if (s->in_flight && stream != s->last_stream)
    return fail(RT_ERR_INVALID, "rt_hip_render: this scene has a launch in flight on another stream (call rt_hip_wait first, "
                                "or use one RtHipScene per concurrent stream)");
  if (s->host.width > 524280u) return fail(RT_ERR_UNSUPPORTED, "frames wider than 524280 pixels");
  RT_HIP_TRY(hipSetDevice(s->device));
  RtHipScene::Slot& sl = s->slot[s->n_launches & 1];
  s->n_launches++;
  sl.rows = local_rows; sl.waves = 0; sl.launched = false;
  sl.samples = (uint64_t)local_rows * s->host.width * spp;
  s->last_stream = stream;
  sl.t_launch = std::chrono::steady_clock::now();
  RT_HIP_TRY(hipMemsetAsync(s->counters.p, 0, 32 * sizeof(unsigned long long), stream));
  // behind the kernel(s) of this launch: its counters into the slot's pinned words (what rt_hip_wait reads)
  auto finish_launch = [&](bool launched) -> int {
    sl.launched = launched; sl.waves = s->last_waves;
    if (launched) RT_HIP_TRY(hipMemcpyAsync(sl.h_counters, s->counters.p, RT_SLOT_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    else std::memset(sl.h_counters, 0, RT_SLOT_COUNTERS * sizeof(unsigned long long));
    RT_HIP_TRY(hipEventRecord(sl.ev_copied, stream));
    s->in_flight = true;
    return RT_OK;
  };
  if (local_rows == 0) return finish_launch(false);

  rtk::KArgs ka;
  ka.sc = s->dev;
  if (s->opt.variant == 1) {  // brute-force arm: no grid, every sphere in the `large` list (object order)
    std::memset(&ka.sc.grid, 0, sizeof ka.sc.grid);
    ka.sc.grid.n_large = s->host.n_spheres;
    ka.sc.large = s->res->sph.all.get<const uint32_t>();
    ka.sc.large_geom = s->res->sph.live.geom.get<const rtc::SphereGeom>();
    ka.sc.n_tris &= ~rtc::FLAT_BVH_BIT;  // (§22: and every flat primitive in file order, the full scan)
  }
  ka.out_rgb8 = (uint8_t*)d_rgb8; ka.out_linear = (float*)d_linear; ka.counters = s->counters.get<unsigned long long>();
  ka.accum = accum; ka.sample_base = sample_base;
#ifdef RT_TEST_PROBES
  ka.probe_rays = g_probe_rays.rays; ka.probe_t = g_probe_rays.t; ka.probe_best = g_probe_rays.best;
#endif
  ka.sc.spp = spp;  // (the kernel's sample count: the pass's, for an accumulating launch)
  ka.queue = (uint32_t*)(s->counters.get<unsigned long long>() + 24);
  ka.local_rows = local_rows;
  const bool tiled = tiles && tiles->tile_rows && tiles->tile_stride;
  ka.tile_rows = tiled ? tiles->tile_rows : 0; ka.first_tile = tiled ? tiles->first_tile : 0;
  ka.tile_stride = tiled ? tiles->tile_stride : 0;
  TileGeom tg;
  { const int rc_geom = tile_geometry(s, local_rows, &tg); if (rc_geom != RT_OK) return rc_geom; }
  const uint32_t tl = tg.tile_log2;
  ka.tile_log2 = tl;
  ka.tile_wl = tg.tile_wl; ka.tile_hl = tg.tile_hl;
  ka.t_slots = rtk::tile_slots(tl);
  ka.tiles_x = tg.tiles_x; s->last_tiles_x = tg.tiles_x;
  ka.n_tiles = tg.tiles_x * tg.tiles_y;
  // a list launch (rt_hip_accumulate_tiles): its queue is the list, mapped to tiles through tile_order
  ka.n_queue = list ? n_list : ka.n_tiles;
  if (list) sl.samples = ((uint64_t)n_list << (2u * tl)) * spp;
  // A tile's samples are handed out to the waves of its workgroup in chunks: an item's latency
  // is what the last wave of a frame waits for, but below ~128 samples per item the acquire /
  // finish overhead shows (measured, profiles/r01_run4_tiles.log): 8x8 -> 8 samples per pixel,
  // 4x4 -> 16, 2x2 -> 32, 1x1 -> 128 — give or take a factor of two so that a frame has about 60
  // items per wave (measured on the whole frame and its 1/2, 1/4, 1/8 shards, profiles/r01_run11_tiles.log:
  // both fewer, larger items and more, smaller ones lose up to 5 %).
  uint32_t chunk_spp = (uint32_t)s->opt.chunk_spp;
  if (chunk_spp == 0) {
    static const uint32_t by_tile[4] = {128u, 32u, 16u, 8u};
    const uint64_t target_items = (uint64_t)s->res->num_cus * rtk::WAVES * 60u;
    const uint64_t ideal = ((uint64_t)ka.n_queue * spp + target_items / 2) / target_items;  // samples per pixel and item (of the tiles queued)
    uint32_t c = 1;
    while ((uint64_t)c * 3u < ideal * 2u) c <<= 1;  // nearest power of two (geometric)
    // (1x1 and 4-pixel tiles never go below their base of 128 samples per item: the 1/8 shard of the headline frame runs 1.678 ms
    //  with chunks of 32 against 1.737 with the 16 the item count alone asks for, profiles/r04_run13_tile_chunk_sweep.log;
    //  16-pixel tiles may: the 800x600 test scene at spp 16 is 3 % faster in two chunks of 8 than in one of 16)
    const uint32_t lo = tl <= 1u ? by_tile[tl] : by_tile[tl] / 2u, hi = by_tile[tl] * 2u;
    chunk_spp = c < lo ? lo : (c > hi ? hi : c);
  }
  if (chunk_spp > spp || spp == 0) chunk_spp = spp ? spp : 1;
  ka.chunk_spp = chunk_spp;
  ka.n_chunks = spp ? (spp + chunk_spp - 1) / chunk_spp : 1;
  const uint32_t n_items = ka.n_queue * ka.n_chunks;
  // Tiles a workgroup takes from the frame's queue per atomic (rt_kernel.hip: wg_stash), at most, and the taper towards
  // single tiles at the end of the frame: remaining tiles / (workgroups x 16).  Measured (profiles/r03_run26_batch_sweep.log):
  // what counts is that ONE wave of a workgroup asks the queue at a time (cover frame at spp 8 / 32 / 128: 1.49 -> 1.15,
  // 3.71 -> 3.35, 12.92 -> 12.80 ms with batches of one); batches of 4 add 5 % on frames of small tiles (test scene 1.09 ->
  // 1.03 ms).  Not more: a batch is a run of the queue's order, and that order puts the deepest tiles first — 8 or 16 of
  // them in one workgroup are the critical path of a short frame (1/8 shard: 1.76 -> 1.87 -> 2.45 ms).
  ka.tile_batch = s->opt.tile_batch > 0 ? (uint32_t)s->opt.tile_batch : 4u;
  ka.batch_share = 16u;
#ifdef RT_DEV_KNOBS
  if (const char* e = std::getenv("RT_BATCH_SHARE")) { const int v = std::atoi(e); if (v >= 1 && v <= 1024) ka.batch_share = (uint32_t)v; }
#endif
  LdsPlan plan;
  { const int rc_plan = plan_lds(s, ka.sc.grid, has_lights, &plan); if (rc_plan != RT_OK) return rc_plan; }
  const bool lds_tables = plan.lds_tables;
  const size_t lds_bytes = plan.lds_bytes;
  ka.sc.light_pool_slots = plan.pool_slots;
  ka.sc.light_base_slots = plan.base_slots;
  ka.sc.light_nest_pool = (uint32_t)s->opt.light_nest_pool;
  ka.sc.light_overflow = nullptr;  // (launch fills it in for the lit kernels)
  s->last_pool_slots = plan.pool_slots; s->last_base_slots = plan.base_slots; s->last_lds_tables = lds_tables; s->last_lds_bytes = lds_bytes;

  // queue order: bottom of the image first; from the second frame of a tile geometry on, the tiles whose samples ran
  // deepest in the previous frame first (their paths are what a frame ends on)
  ka.order_mode = s->opt.order_mode != 0 ? 1u : 0u;
  ka.tile_order = nullptr; ka.tile_depth = nullptr;
  // XCD affinity: runs of 1.5 KB of a scanline's tiles (512 pixels) per XCD, for large frames (smaller ones — the shards
  // of the headline frame — lose more to the coarser balance than the write traffic is worth: 2.10 instead of 1.89 ms,
  // profiles/r02_run29_affinity.log)
  ka.aff_group_log2 = 0xFFFFFFFFu;
  for (int x = 0; x < 8; ++x) { ka.xcd_cnt[x] = 0; ka.xcd_off[x] = 0; }
  {
#ifdef RT_DEV_KNOBS  // (A/B builds only: tools/affinity_sweep.sh)
    static const uint32_t run_px_log2 = [] { const char* e = std::getenv("RT_AFF_RUN_LOG2"); const int v = e ? std::atoi(e) : 9; return (uint32_t)(v < 3 ? 3 : (v > 14 ? 14 : v)); }();
#else
    constexpr uint32_t run_px_log2 = 9;  // runs of 512 pixels of a tile row (profiles/r02_run29_affinity.log)
#endif
    const uint32_t gl = ka.tile_wl >= run_px_log2 ? 0u : run_px_log2 - ka.tile_wl;
    const uint32_t n_groups = (ka.n_tiles + (1u << gl) - 1u) >> gl;
    // on for frames of at least 2^19 pixels (the headline frame: 0.96 M; its 1/2 ... 1/8 shards and the 800x600 test scene are
    // below and lose 6 - 15 % to the coarser balance, profiles/r03_run8_shard_affinity_sweep.log) with at least 8 runs
    const bool big = (uint64_t)local_rows * s->host.width >= (1ull << 19);
    // (list launches: off — their queue is the caller's list, not the frame's runs; DESIGN.md §11 has the A/B)
    if (!list && ((s->opt.tile_affinity == 1 && big && n_groups >= 8u) || (s->opt.tile_affinity == 2 && n_groups >= 8u))) {
      ka.aff_group_log2 = gl;
      for (uint32_t g = 0; g < 8u && g < n_groups; ++g) {  // groups g, g + 8, ...: all full but possibly the frame's last
        const uint32_t mine = (n_groups - 1u - g) / 8u + 1u;
        const uint32_t last = g + 8u * (mine - 1u);
        const uint32_t last_size = last == n_groups - 1u ? ka.n_tiles - (last << gl) : (1u << gl);
        ka.xcd_cnt[g] = ((mine - 1u) << gl) + last_size;
      }
      for (int x = 1; x < 8; ++x) ka.xcd_off[x] = ka.xcd_off[x - 1] + ka.xcd_cnt[x - 1];
    }
  }
  if (list) {  // the list is the queue, in the caller's order; no depths are measured
    ka.order_mode = 1u;
    ka.tile_order = list;
  } else if (s->opt.order_mode >= 2) {
    RtHipScene::OrderKey key;
    key.n_tiles = ka.n_tiles; key.tile_log2 = tl; key.tile_shape = (uint32_t)s->opt.tile_shape; key.aff_group_log2 = ka.aff_group_log2;
    key.tile_rows = ka.tile_rows; key.first_tile = ka.first_tile; key.tile_stride = ka.tile_stride; key.local_rows = local_rows;
    int rc;
    if ((rc = s->order.tile_depth.ensure((size_t)ka.n_tiles * 4)) != RT_OK || (rc = s->order.tile_order.ensure((size_t)ka.n_tiles * 4)) != RT_OK) return rc;
    if (!(key == s->order.key)) { s->order.key = key; s->order.forget(); }
    // The order of THIS frame from the depths the previous frame of the SAME view measured (sorted here, stream-ordered ahead of
    // the launch — until round 5 behind the frame that measured them, which an animation paid every frame for an order it never
    // used).  Which tiles breed deep paths is a property of scene and camera: rebuilt after each of a view's first two frames,
    // then kept; rt_hip_set_camera with a different camera starts over WITHOUT an order (below).
    if (s->order.fresh) {
      hipLaunchKernelGGL(rtk::rt_order_tiles, dim3(1), dim3(1024), 0, stream, s->order.tile_depth.get<const uint32_t>(), s->order.tile_order.get<uint32_t>(), ka.n_tiles, ka.aff_group_log2);
      RT_HIP_TRY(hipGetLastError());
      s->order.ready = true; s->order.fresh = false;
    }
    if (s->opt.order_mode == 2 && s->order.age < 2) ka.tile_depth = s->order.tile_depth.get<uint32_t>();  // (measured only while the order is still being built)
#ifdef RT_TEST_PROBES
    if (ka.probe_rays) ka.tile_depth = nullptr;  // (a probe frame's depths say nothing about the view: it measures none)
#endif
    if (s->order.ready) ka.tile_order = s->order.tile_order.get<uint32_t>();
  }

  Kernel k;
  int rc;
  if ((rc = select_kernel(s, has_lights, lds_tables, ka.sc.grid.wide != 0u, accum != nullptr, &k)) != RT_OK) return rc;
  if ((rc = prepare(s, k, lds_bytes, stream)) != RT_OK) return rc;  // (host-side set-up: before the start event)
  RT_HIP_TRY(hipEventRecord(sl.ev_start, stream));
  // A frame without a measured order (the first of a scene, a one-shot render) leaves the queue bottom row first and ends on
  // whatever deep path started last: 13.3 instead of 12.8 ms on the headline frame.  Two ways to SEED an order — a depth guess
  // from the spheres' projections, a one-sample probe launch — were built and measured in round 4, both slower than no seed
  // (profiles/r04_run3_first_frame_orders.log; the code: profiles/r05_order_seed_removed.patch): what the measured order
  // knows is WHICH tiles hold one of the rare 50-segment paths, which a replay of the same seeds predicts and nothing cheaper does.
  launch(s, k, ka, lds_bytes, n_items, stream);
  RT_HIP_TRY(hipGetLastError());
  RT_HIP_TRY(hipEventRecord(sl.ev_stop, stream));
  if (ka.tile_depth) { s->order.age++; s->order.fresh = true; }  // (the NEXT frame of this view sorts them into its order)
  return finish_launch(true);
}
}  // namespace

extern "C" int rt_hip_render(RtHipScene* s, const RtRowTiles* tiles, void* d_rgb8, void* d_linear, void* stream_) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  if (!d_rgb8 && rt_tiles_local_rows(s->host.height, tiles) != 0) return fail(RT_ERR_INVALID, "null framebuffer");
  // the exact pixel sums are 2^-40 fixed point in 64 bits: spp * 2^40 must stay below 2^63
  if (s->host.samples_per_pixel > (1u << 22)) return fail(RT_ERR_UNSUPPORTED, "more than 2^22 samples per pixel");
  return launch_frame(s, tiles, d_rgb8, d_linear, nullptr, 0u, s->host.samples_per_pixel, stream_);
}

// Progressive rendering.  Sample s of pixel p traces the same path whatever the frame's sample count (Philox is addressed by
// (pixel, sample index, node, slot)), and a pixel's sum is exact fixed point (integer adds: any order, any grouping), so the sums
// of any set of passes covering [0, N) resolved over N are the one-shot frame at N samples, bit for bit.
namespace {
int check_accum(const RtHipScene* s, const RtRowTiles* tiles, const void* d_accum) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  if (rt_tiles_local_rows(s->host.height, tiles) == 0) return RT_OK;
  if (!d_accum) return fail(RT_ERR_INVALID, "null accumulator");
  return check_aligned(d_accum, 8, "the accumulator must be 8-byte aligned");
}
// rt_resolve over the n_px pixels of d_accum: every pixel over n_samples, or (d_tile_spp != nullptr) each over its tile's count d_tile_spp[id],
// the tiles those of tg.  Arguments checked by the caller; nothing to write: nothing launched.
int launch_resolve(RtHipScene* s, const void* d_accum, uint64_t n_px, uint32_t n_samples, const uint32_t* d_tile_spp, const TileGeom& tg, void* d_rgb8,
                   void* d_linear, void* stream) {
  if (!d_rgb8 && !d_linear) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  const uint64_t blocks = ((n_px + 3u) / 4u + 255u) / 256u;
  if (blocks > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, "frame too large to resolve");
  hipLaunchKernelGGL(rtk::rt_resolve, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)d_accum, n_samples, n_px,
                     (uint8_t*)d_rgb8, (float*)d_linear, d_tile_spp, d_tile_spp ? s->host.width : 0u, tg.tiles_x, tg.tile_wl, tg.tile_hl);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
}  // namespace

extern "C" int rt_hip_accumulate(RtHipScene* s, const RtRowTiles* tiles, uint32_t sample_begin, uint32_t sample_count, void* d_accum, void* stream) {
  const int rc = check_accum(s, tiles, d_accum);
  if (rc != RT_OK) return rc;
  if (sample_count == 0) return fail(RT_ERR_INVALID, "sample_count must be at least 1");
  if (const int refused = check_samples(sample_begin, sample_count)) return refused;
  return launch_frame(s, tiles, nullptr, nullptr, (unsigned long long*)d_accum, sample_begin, sample_count, stream);
}

extern "C" int rt_hip_resolve(RtHipScene* s, const RtRowTiles* tiles, const void* d_accum, uint32_t n_samples, void* d_rgb8, void* d_linear, void* stream) {
  int rc = check_accum(s, tiles, d_accum);
  if (rc != RT_OK) return rc;
  if (n_samples == 0) return fail(RT_ERR_INVALID, "n_samples must be at least 1");
  if ((rc = check_samples(0, n_samples)) != RT_OK) return rc;
  if ((rc = check_aligned(d_linear, 4, "d_linear must be 4-byte aligned")) != RT_OK) return rc;
  const uint64_t n_px = (uint64_t)rt_tiles_local_rows(s->host.height, tiles) * s->host.width;
  if (n_px == 0) return RT_OK;
  return launch_resolve(s, d_accum, n_px, n_samples, nullptr, TileGeom(), d_rgb8, d_linear, stream);
}

// Adaptive sampling: per-tile sample counts over the accumulating kernels' own pixel tiles.
namespace {
// the tiles of `tiles`' packed rows; n_list must name 1 .. tile count tiles
int check_list(const RtHipScene* s, const RtRowTiles* tiles, const uint32_t* d_list, uint32_t n_list, TileGeom* tg) {
  if (!d_list || n_list == 0) return fail(RT_ERR_INVALID, "the tile list must name at least one tile");
  if (const int refused = check_aligned(d_list, 4, "the tile list must be 4-byte aligned")) return refused;
  const int rc = tile_geometry(s, rt_tiles_local_rows(s->host.height, tiles), tg);
  if (rc != RT_OK) return rc;
  if ((uint64_t)n_list > (uint64_t)tg->tiles_x * tg->tiles_y) return fail(RT_ERR_INVALID, "the tile list is longer than the frame has tiles");
  return RT_OK;
}
}  // namespace

extern "C" int rt_hip_tile_grid(const RtHipScene* s, const RtRowTiles* tiles, uint32_t out[4]) {
  if (!s || !out) return fail(RT_ERR_INVALID, "null argument");
  TileGeom tg;
  const int rc = tile_geometry(s, rt_tiles_local_rows(s->host.height, tiles), &tg);
  if (rc != RT_OK) return rc;
  out[0] = 1u << tg.tile_wl; out[1] = 1u << tg.tile_hl; out[2] = tg.tiles_x; out[3] = tg.tiles_y;
  return RT_OK;
}

extern "C" int rt_hip_accumulate_tiles(RtHipScene* s, const RtRowTiles* tiles, const uint32_t* d_tile_list, uint32_t n_list, uint32_t sample_begin,
                                       uint32_t sample_count, void* d_accum, void* stream) {
  int rc = check_accum(s, tiles, d_accum);
  if (rc != RT_OK) return rc;
  TileGeom tg;
  if ((rc = check_list(s, tiles, d_tile_list, n_list, &tg)) != RT_OK) return rc;
  if (!d_accum) return fail(RT_ERR_INVALID, "null accumulator");
  if (sample_count == 0) return fail(RT_ERR_INVALID, "sample_count must be at least 1");
  if ((rc = check_samples(sample_begin, sample_count)) != RT_OK) return rc;
  return launch_frame(s, tiles, nullptr, nullptr, (unsigned long long*)d_accum, sample_begin, sample_count, stream, d_tile_list, n_list);
}

extern "C" int rt_hip_tile_error(RtHipScene* s, const RtRowTiles* tiles, const uint32_t* d_tile_list, uint32_t n_list, const void* d_now, uint32_t n_now,
                                 const void* d_prev, uint32_t n_prev, double* d_tile_err, void* stream) {
  if (!s || !d_now || !d_prev || !d_tile_err) return fail(RT_ERR_INVALID, "null argument");
  TileGeom tg;
  int rc = check_list(s, tiles, d_tile_list, n_list, &tg);
  if (rc != RT_OK) return rc;
  for (const void* q : {d_now, d_prev, (const void*)d_tile_err})
    if ((rc = check_aligned(q, 8, "accumulators and the error array must be 8-byte aligned")) != RT_OK) return rc;
  if (n_prev == 0 || n_now <= n_prev) return fail(RT_ERR_INVALID, "the counts must satisfy 0 < n_prev < n_now");
  if ((rc = check_samples(0, n_now)) != RT_OK) return rc;
  RT_HIP_TRY(hipSetDevice(s->device));
  const uint64_t threads = (uint64_t)n_list << (2u * tg.tile_log2), blocks = (threads + 255u) / 256u;
  hipLaunchKernelGGL(rtk::rt_tile_error, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)d_now, n_now,
                     (const unsigned long long*)d_prev, n_prev, d_tile_list, n_list, tg.tile_log2, tg.tile_wl, tg.tile_hl, tg.tiles_x,
                     tg.tiles_x * tg.tiles_y, s->host.width, rt_tiles_local_rows(s->host.height, tiles), d_tile_err);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_hip_resolve_tiles(RtHipScene* s, const RtRowTiles* tiles, const void* d_accum, const uint32_t* d_tile_spp, void* d_rgb8, void* d_linear,
                                    void* stream) {
  int rc = check_accum(s, tiles, d_accum);
  if (rc != RT_OK) return rc;
  const uint32_t rows = rt_tiles_local_rows(s->host.height, tiles);
  if (rows == 0) return RT_OK;
  if (!d_tile_spp) return fail(RT_ERR_INVALID, "null tile counts");
  if ((rc = check_aligned(d_tile_spp, 4, "the tile counts must be 4-byte aligned")) != RT_OK) return rc;
  if ((rc = check_aligned(d_linear, 4, "d_linear must be 4-byte aligned")) != RT_OK) return rc;
  TileGeom tg;
  if ((rc = tile_geometry(s, rows, &tg)) != RT_OK) return rc;
  return launch_resolve(s, d_accum, (uint64_t)rows * s->host.width, 1u, d_tile_spp, tg, d_rgb8, d_linear, stream);
}

#ifdef RT_TEST_PROBES
// Diagnostics: the per-tile path depths the last measuring frame left behind (tile_order 2, first two frames of a view):
// out[tile] = deepest camera path seen in the tile, tiles in row-major order of the launch's tile grid (*tiles_x wide).
// Returns the number of tiles copied (at most cap), or a negative RtStatus.
extern "C" int rt_hip_debug_tile_depth(RtHipScene* s, uint32_t* out, uint32_t cap, uint32_t* tiles_x) {
  if (!s || !out) return fail(RT_ERR_INVALID, "null argument");
  RT_HIP_TRY(hipSetDevice(s->device));
  if (s->n_launches) RT_HIP_TRY(hipStreamSynchronize(s->last_stream));
  const uint32_t n = s->order.key.n_tiles < cap ? s->order.key.n_tiles : cap;
  if (n && s->order.tile_depth.p) RT_HIP_TRY(hipMemcpy(out, s->order.tile_depth.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (tiles_x) *tiles_x = s->last_tiles_x;
  return (int)n;
}

extern "C" int rt_hip_debug_timeline(RtHipScene* s, uint64_t* out, uint32_t max_waves) {
  if (!s || !out) return fail(RT_ERR_INVALID, "null argument");
  RT_HIP_TRY(hipSetDevice(s->device));
  RT_HIP_TRY(hipStreamSynchronize(s->last_stream));
  const uint32_t n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(s->last_waves, max_waves), RT_TIMELINE_WAVES);
  RT_HIP_TRY(hipMemcpy(out, s->counters.p, (32 + (size_t)n * 4) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return (int)n;
}

#endif  // RT_TEST_PROBES

namespace {
// the report of the launch that used `sl` (its counter copy must have completed: the caller synchronised)
void fill_stats(const RtHipScene* s, const RtHipScene::Slot& sl, RtStats* stats) {
  std::memset(stats, 0, sizeof *stats);
  stats->n_gpus_used = 1;
  const unsigned long long* c = sl.h_counters;  // segments, exact tests, tex_oob, grid steps, 4 x wave trip counts, 8 x section cycles, profile clocks
  float ms = 0.f;
  if (sl.launched && hipEventElapsedTime(&ms, sl.ev_start, sl.ev_stop) != hipSuccess) { ms = 0.f; (void)hipGetLastError(); }
  stats->samples = sl.samples;
  stats->segments = c[0];
  stats->sphere_tests = c[0] * (uint64_t)s->host.n_spheres;
  stats->exact_tests = c[1];
  stats->tex_oob = c[2];
  stats->grid_steps = c[3];
  stats->segments_repeated = c[28] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c[28];
  for (int k = 0; k < 4; ++k) stats->wave_iters[k] = c[4 + k];
  for (int k = 0; k < 8; ++k) stats->prof_cycles[k] = c[8 + k];
  if (c[14] && sl.waves) {  // profile builds: longest / shortest wave, waves launched
    stats->prof_cycles[7] = c[15];
    stats->prof_cycles[8] = ~c[17];
    stats->prof_cycles[10] = sl.waves;
  }
  stats->kernel_ms = ms;
  stats->frame_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - sl.t_launch).count();
}
// wait for ONE launch — the one that used slot `which` — and report it (the group's pipelined frames: frame i is collected
// while frame i+1 is in flight on the same stream)
int wait_slot(RtHipScene* s, int which, RtStats* stats) {
  RT_HIP_TRY(hipSetDevice(s->device));
  RtHipScene::Slot& sl = s->slot[which & 1];
  RT_HIP_TRY(hipEventSynchronize(sl.ev_copied));
  if (&sl == &s->last_slot()) s->in_flight = false;
  if (stats) fill_stats(s, sl, stats);
  return RT_OK;
}
}  // namespace

extern "C" int rt_hip_wait(RtHipScene* s, RtStats* stats) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  RT_HIP_TRY(hipSetDevice(s->device));
  if (s->n_launches == 0) { if (stats) { std::memset(stats, 0, sizeof *stats); stats->n_gpus_used = 1; } return RT_OK; }
  RT_HIP_TRY(hipStreamSynchronize(s->last_stream));
  s->in_flight = false;
  if (stats) fill_stats(s, s->last_slot(), stats);
  return RT_OK;
}

// what a resident scene was built into (diagnostics; bench.py prices the tables' bytes with it)
extern "C" int64_t rt_hip_scene_query(const RtHipScene* s, const char* key) {
  if (!s || !key) return -1;
  if (!std::strcmp(key, "n_spheres")) return (int64_t)s->host.n_spheres;
  if (!std::strcmp(key, "n_lights")) return (int64_t)s->dev.n_lights;
  if (!std::strcmp(key, "grid_cells")) return (int64_t)s->res->sph.live.grid.n_cells;       // padded cell table (8 B each; wide tables: 16 B)
  if (!std::strcmp(key, "grid_items")) return (int64_t)s->res->sph.live.grid.n_items;       // u16 each (wide tables: u32)
  if (!std::strcmp(key, "grid_wide")) return (int64_t)s->res->sph.live.grid.wide;           // 1: 32-bit item lists (more than 65 535 spheres)
  if (!std::strcmp(key, "grid_large")) return (int64_t)s->res->sph.live.grid.n_large;
  if (!std::strcmp(key, "texel_bytes")) return (int64_t)s->res->texel_bytes;       // 4-byte texels of textures + sky resident in HBM
  if (!std::strcmp(key, "light_pool_slots")) return (int64_t)s->last_pool_slots;  // of the last launch: records in the pools of light frames /
  if (!std::strcmp(key, "light_base_slots")) return (int64_t)s->last_base_slots;  // colour-map bases, the kernel's dynamic LDS, tables staged in LDS
  if (!std::strcmp(key, "lds_bytes")) return (int64_t)s->last_lds_bytes;
  if (!std::strcmp(key, "lds_tables")) return (int64_t)s->last_lds_tables;
  if (!std::strcmp(key, "triangles")) return (int64_t)s->res->flat.n_tris;      // of "quads", the entries of shape triangle
  if (!std::strcmp(key, "flat_bvh")) return (int64_t)s->res->flat.n_nodes;  // nodes of the structure over the flat primitives; 0: none
  if (!std::strcmp(key, "flat_motion")) return (int64_t)s->res->flat.n_moving;  // entries that move within the frame; 0: none
  if (!std::strcmp(key, "flat_lights")) return (int64_t)s->res->flat_lights.size();  // entries that emit; "n_lights" counts them too
  if (!std::strcmp(key, "flat_images")) return (int64_t)s->res->flat.n_images;   // entries that carry an image; 0: none
  if (!std::strcmp(key, "flat_normals")) return (int64_t)s->res->flat.n_normals;  // entries that carry shading normals; 0: none
  if (!std::strcmp(key, "flat_refits")) return (int64_t)s->res->flat.refits;  // updates applied by refit since the structure was last built
  if (!std::strcmp(key, "flat_build")) return (int64_t)s->opt.flat_build;  // the option: 1: a rebuild the caller asks for runs on the device
  if (!std::strcmp(key, "flat_device_builds")) return (int64_t)s->res->flat.device_builds;  // order tables built on the device since creation
  if (!std::strcmp(key, "quads")) return (int64_t)s->res->flat.n_quads;         // flat parallelograms (rt_hip_scene_create_quads)
  if (!std::strcmp(key, "last_kernel")) return (int64_t)s->last_kernel;   // QUADS 512 | SOLID 256 | MEDIUM 128 | MOTION 64 | LENS 32 | ACCUM 16 | WIDE 8 | HL 4 | SIMPLE 2 | LDS 1; -1 before the first launch
  if (!std::strcmp(key, "media")) return (int64_t)s->res->n_media;         // spheres of kind RT_MAT_MEDIUM
  if (!std::strcmp(key, "solids")) return (int64_t)s->res->n_solids;       // spheres of kind RT_MAT_CHECKER or RT_MAT_NOISE
  if (!std::strcmp(key, "motion")) return (int64_t)s->res->sph.live.n_moving;       // spheres that move over the shutter (rt_hip_scene_create_moving); 0: static
  if (!std::strcmp(key, "lens")) return s->dev.lens_r != 0.0 ? 1 : 0;    // 1: a thin lens is set (rt_hip_set_lens), 0: the pinhole
  if (!std::strcmp(key, "accum_samples")) return (int64_t)s->prog.samples;
  if (!std::strcmp(key, "temporal_surface")) return s->tp.surface ? 1 : 0;
  // the last rt_hip_render_adaptive_to_host: its rounds, and round i's tiles, samples per pixel after it, kernel time in microseconds
  if (!std::strcmp(key, "adaptive_rounds")) return (int64_t)s->ad.rounds.size();
  for (const char* f : {"adaptive_round_tiles_", "adaptive_round_spp_", "adaptive_round_kernel_us_"}) {
    const size_t l = std::strlen(f);
    if (std::strncmp(key, f, l) != 0 || key[l] < '0' || key[l] > '9') continue;
    const unsigned long i = std::strtoul(key + l, nullptr, 10);
    if (i >= s->ad.rounds.size()) return -1;
    const RtHipScene::Adaptive::Round& r = s->ad.rounds[i];
    return f[15] == 't' ? (int64_t)r.tiles : (f[15] == 's' ? (int64_t)r.spp : (int64_t)std::llround(r.kernel_ms * 1000.0));
  }  // samples per pixel in the scene's accumulator (rt_hip_refine_to_host)
  if (!std::strcmp(key, "table_bytes")) return (int64_t)((size_t)s->host.n_spheres * (sizeof(rtc::SphereGeom) + sizeof(rtc::MatCore)) + (size_t)s->res->sph.live.grid.n_cells * (s->res->sph.live.grid.wide ? 16u : 8u) + (size_t)s->res->sph.live.grid.n_items * (s->res->sph.live.grid.wide ? 4u : 2u));
  return -1;
}

extern "C" int rt_hip_set_camera(RtHipScene* s, const double origin[3], const double lower_left[3], const double horizontal[3],
                                 const double vertical[3]) {
  if (!s || !origin || !lower_left || !horizontal || !vertical) return fail(RT_ERR_INVALID, "null argument");
  s->prog.reset();  // (whatever the camera: a progressive frame starts over)
  bool same = true;
  for (int i = 0; i < 3; ++i)
    same = same && s->host.cam_origin[i] == origin[i] && s->host.cam_lower_left[i] == lower_left[i] && s->host.cam_horizontal[i] == horizontal[i] &&
           s->host.cam_vertical[i] == vertical[i];
  if (same) return RT_OK;  // (the same view: its order stays)
  for (int i = 0; i < 3; ++i) {
    s->host.cam_origin[i] = s->dev.cam_origin[i] = origin[i];
    s->host.cam_lower_left[i] = s->dev.cam_ll[i] = lower_left[i];
    s->host.cam_horizontal[i] = s->dev.cam_h[i] = horizontal[i];
    s->host.cam_vertical[i] = s->dev.cam_v[i] = vertical[i];
  }
  // A new view starts WITHOUT an order (bottom row first) and measures its own.  Until round 5 the previous view's order stayed
  // in use ("the views of an animation are close") — measured in round 6 on the headline scene turning 3 degrees per frame:
  // the stale order costs 3 - 10 % against the view's own order and is WORSE than no order (+3 - 4 %): the tiles that hold a
  // view's rare 50-segment paths are 4x4 pixels, and a 3 degree turn moves the spheres by tens of pixels
  // (bench.py `animation.same_views`, profiles/r06_run*_bench.json; the old arm was removed after that A/B).
  s->order.forget();
  return RT_OK;
}

extern "C" int rt_hip_set_lens(RtHipScene* s, const double u[3], const double v[3], double lens_radius) {
  if (!s || !u || !v) return fail(RT_ERR_INVALID, "null argument");
  if (!(lens_radius >= 0.0 && lens_radius <= 1.7976931348623157e308)) return fail(RT_ERR_INVALID, "lens_radius must be finite and >= 0");
  bool same = lens_radius == s->dev.lens_r;
  if (lens_radius != 0.0)
    for (int i = 0; i < 3; ++i) same = same && s->dev.lens_u[i] == u[i] && s->dev.lens_v[i] == v[i];
  if (same) return RT_OK;  // (pinhole to pinhole, or the same lens: the accumulator and the queue order stay)
  for (int i = 0; i < 3; ++i) { s->dev.lens_u[i] = u[i]; s->dev.lens_v[i] = v[i]; }
  s->dev.lens_r = lens_radius;
  s->prog.reset();
  s->order.forget();  // (another view: it measures its own order, as after rt_hip_set_camera)
  return RT_OK;
}

namespace {
// What the blocking host forms share.  They render into s->frame on the NULL stream: the clock and the device at the start; at the end the
// wait for the form's launches, then the frame copied to the caller with the last launch's stats, frame_ms taken from the form's own start.
struct HostForm {
  RtHipScene* s;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  RtStats st{};   // of the form's last launch (wait)
  int begin() { RT_HIP_TRY(hipSetDevice(s->device)); return RT_OK; }
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  int wait(int rc) { return rc == RT_OK ? rt_hip_wait(s, &st) : rc; }  // rc: how enqueueing went; a form that failed drops its own state
  int deliver(uint8_t* out_rgb8, RtStats* stats) {
    RT_HIP_TRY(hipMemcpy(out_rgb8, s->frame.p, (size_t)s->host.width * s->host.height * 3, hipMemcpyDeviceToHost));
    if (stats) { *stats = st; stats->frame_ms = ms(); }
    return RT_OK;
  }
};
}  // namespace

extern "C" int rt_hip_render_to_host(RtHipScene* s, uint8_t* out_rgb8, RtStats* stats) {
  if (!s || !out_rgb8) return fail(RT_ERR_INVALID, "null argument");
  HostForm f{s};
  int rc = f.begin();
  if (rc == RT_OK) rc = s->frame.ensure((size_t)s->host.width * s->host.height * 3);
  if (rc == RT_OK) rc = rt_hip_render(s, nullptr, s->frame.p, nullptr, nullptr);
  if ((rc = f.wait(rc)) != RT_OK) return rc;
  return f.deliver(out_rgb8, stats);
}

namespace {
int denoise_frame(RtHipScene* s, const void* d_linear, const void* d_aov, uint32_t iterations, const float sigma[4], void* d_out_linear,
                  void* d_out_rgb8, hipStream_t stream, bool in4 = false);
// the host form's AOV sample count: min(RT_DENOISE_AOV_SAMPLES, samples per pixel), at least 1
uint32_t aov_default_samples(uint32_t spp) { return spp < 1u ? 1u : (spp < RT_DENOISE_AOV_SAMPLES ? spp : RT_DENOISE_AOV_SAMPLES); }
// Progressive rendering into the scene's own accumulator, blocking: the next sample_count samples of every pixel, then the whole
// accumulator resolved to RGB8 in out_rgb8.  Passes and the resolve run on the NULL stream, like rt_hip_render_to_host.
// iterations >= 0 (rt_hip_refine_to_host_denoised): the resolve goes to linear f32 and is denoised over the AOVs of the
// accumulator's start, aov_default_samples(spp) samples of them, computed once per start.
int refine_to_host(RtHipScene* s, uint32_t sample_count, int iterations, uint8_t* out_rgb8, RtStats* stats) {
  if (!s || !out_rgb8) return fail(RT_ERR_INVALID, "null argument");
  if (sample_count == 0) return fail(RT_ERR_INVALID, "sample_count must be at least 1");
  if (const int refused = check_samples(s->prog.samples, sample_count)) return refused;
  HostForm f{s};
  int rc = f.begin();
  if (rc != RT_OK) return rc;
  const size_t px = (size_t)s->host.width * s->host.height, bytes = px * 3;
  bool grew = false;
  if ((rc = s->prog.accum.ensure(px * 24, &grew)) != RT_OK) return rc;
  if (grew) s->prog.reset();
  if ((rc = s->frame.ensure(bytes)) != RT_OK) return rc;
  if (iterations >= 0) {  // the host form's own linear frame and AOV record
    if ((rc = s->prog.dn_lin.ensure(px * 12)) != RT_OK || (rc = s->prog.dn_aov.ensure(px * 32, &grew)) != RT_OK) return rc;
    if (grew) s->prog.aov_ready = false;
  }
  if (s->prog.zero && px) { RT_HIP_TRY(hipMemsetAsync(s->prog.accum.p, 0, px * 24, nullptr)); s->prog.zero = false; }
  const uint32_t n = s->prog.samples + sample_count;
  unsigned long long* accum = s->prog.accum.get<unsigned long long>();
  rc = rt_hip_accumulate(s, nullptr, s->prog.samples, sample_count, accum, nullptr);
  if (iterations < 0) {
    if (rc == RT_OK) rc = rt_hip_resolve(s, nullptr, accum, n, s->frame.p, nullptr, nullptr);
  } else {
    if (rc == RT_OK && !s->prog.aov_ready) {
      rc = rt_hip_render_aovs(s, nullptr, aov_default_samples(s->host.samples_per_pixel), s->prog.dn_aov.p, nullptr);
      if (rc == RT_OK) s->prog.aov_ready = true;
    }
    if (rc == RT_OK) rc = rt_hip_resolve(s, nullptr, accum, n, nullptr, s->prog.dn_lin.p, nullptr);
    const float sigma[4] = {RT_DENOISE_SIGMA_COLOR, RT_DENOISE_SIGMA_NORMAL, RT_DENOISE_SIGMA_ALBEDO, RT_DENOISE_SIGMA_INV_DEPTH};
    if (rc == RT_OK) rc = denoise_frame(s, s->prog.dn_lin.p, s->prog.dn_aov.p, (uint32_t)iterations, sigma, nullptr, s->frame.p, nullptr);
  }
  if ((rc = f.wait(rc)) != RT_OK) { s->prog.reset(); return rc; }  // (a pass that did not complete leaves the accumulator unknown: start over)
  s->prog.samples = n;
  return f.deliver(out_rgb8, stats);
}
}  // namespace

extern "C" int rt_hip_refine_to_host(RtHipScene* s, uint32_t sample_count, uint8_t* out_rgb8, RtStats* stats) {
  return refine_to_host(s, sample_count, -1, out_rgb8, stats);
}

// ---------------------------------------------------------------------------------------------------- denoising
namespace {
int check_whole_frame(const RtHipScene* s, const RtRowTiles* tiles) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  if (tiles) return fail(RT_ERR_UNSUPPORTED, "denoising works on whole frames only: tiles must be NULL");
  if (s->host.height > 65535u * 16u) return fail(RT_ERR_UNSUPPORTED, "frames taller than 1 048 560 rows");
  return RT_OK;
}
int check_sigmas(const float sigma[4]) {
  for (int i = 0; i < 4; ++i)
    if (!(sigma[i] > 0.0f) || !(sigma[i] <= 3.4028234663852886e38f)) return fail(RT_ERR_INVALID, "every sigma must be finite and greater than 0");
  return RT_OK;
}
dim3 px_grid(const RtHipScene* s) { return dim3((s->host.width + 15u) / 16u, (s->host.height + 15u) / 16u); }
// the L iterations: input -> ping -> pong -> ... -> outputs; arguments checked by the caller.  in4: the input is f32 x 4 per pixel (a
// temporal history: its rgb is filtered, its fourth float ignored) and goes through the instantiations that read the ping-pong
int denoise_frame(RtHipScene* s, const void* d_linear, const void* d_aov, uint32_t iterations, const float sigma[4], void* d_out_linear,
                  void* d_out_rgb8, hipStream_t stream, bool in4) {
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px == 0 || (!d_out_linear && !d_out_rgb8)) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  if (iterations >= 2) { const int rc = s->dn_ping.ensure(2 * px * 16); if (rc != RT_OK) return rc; }
  float4* const buf[2] = {s->dn_ping.get<float4>(), s->dn_ping.get<float4>() + px};
  const float4* aov = (const float4*)d_aov;
  const uint32_t W = s->host.width, H = s->host.height;
  const dim3 grid = px_grid(s), block(16, 16);
  if (iterations == 0) {
    if (in4) hipLaunchKernelGGL((rtk::rt_denoise<true, true>), grid, block, 0, stream, (const float*)d_linear, aov, W, H, 0u, rtc::DenoiseK{},
                                (float4*)nullptr, (float*)d_out_linear, (uint8_t*)d_out_rgb8);
    else hipLaunchKernelGGL((rtk::rt_denoise<false, true>), grid, block, 0, stream, (const float*)d_linear, aov, W, H, 0u, rtc::DenoiseK{},
                            (float4*)nullptr, (float*)d_out_linear, (uint8_t*)d_out_rgb8);
    RT_HIP_TRY(hipGetLastError());
    return RT_OK;
  }
  for (uint32_t i = 0; i < iterations; ++i) {
    const rtc::DenoiseK k = rtc::denoise_consts(i, sigma[0], sigma[1], sigma[2], sigma[3]);
    const bool first = i == 0 && !in4, last = i + 1 == iterations;
    const float* in = i == 0 ? (const float*)d_linear : (const float*)buf[(i - 1) & 1];
    float4* out4 = last ? nullptr : buf[i & 1];
    float* ol = last ? (float*)d_out_linear : nullptr;
    uint8_t* ob = last ? (uint8_t*)d_out_rgb8 : nullptr;
    if (first && last) hipLaunchKernelGGL((rtk::rt_denoise<false, true>), grid, block, 0, stream, in, aov, W, H, 1u << i, k, out4, ol, ob);
    else if (first) hipLaunchKernelGGL((rtk::rt_denoise<false, false>), grid, block, 0, stream, in, aov, W, H, 1u << i, k, out4, ol, ob);
    else if (last) hipLaunchKernelGGL((rtk::rt_denoise<true, true>), grid, block, 0, stream, in, aov, W, H, 1u << i, k, out4, ol, ob);
    else hipLaunchKernelGGL((rtk::rt_denoise<true, false>), grid, block, 0, stream, in, aov, W, H, 1u << i, k, out4, ol, ob);
    RT_HIP_TRY(hipGetLastError());
  }
  return RT_OK;
}
// The feature kernels by the four feature bits of the megakernel's key, (SOLID | MEDIUM | MOTION | LENS) / LENS; the second table: the same
// sixteen with the QUADS arm, for scenes that hold a quad
using AovKernel = void (*)(const rtc::DevScene, uint32_t, float4*);
template <int... F> std::array<AovKernel, 16> aov_kernels(std::integer_sequence<int, F...>) {
  return {rtk::rt_aov<(F & 1) != 0, (F & 2) != 0, (F & 4) != 0, (F & 8) != 0>...};
}
template <int... F> std::array<AovKernel, 16> aov_quads_kernels(std::integer_sequence<int, F...>) {
  return {rtk::rt_aov_quads<(F & 1) != 0, (F & 2) != 0, (F & 4) != 0, (F & 8) != 0>...};
}
}  // namespace

extern "C" int rt_hip_render_aovs(RtHipScene* s, const RtRowTiles* tiles, uint32_t n_samples, void* d_aov, void* stream) {
  const int rc = check_whole_frame(s, tiles);
  if (rc != RT_OK) return rc;
  if (n_samples == 0) return fail(RT_ERR_INVALID, "n_samples must be at least 1");
  if (const int refused = check_samples(0, n_samples, "")) return refused;
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px == 0) return RT_OK;
  if (!d_aov) return fail(RT_ERR_INVALID, "null AOV buffer");
  if (const int refused = check_aligned(d_aov, 16, "the AOV buffer must be 16-byte aligned")) return refused;
  RT_HIP_TRY(hipSetDevice(s->device));
  static const std::array<AovKernel, 16> table = aov_kernels(std::make_integer_sequence<int, 16>());
  const int features = (s->res->n_solids ? rtk::KEY_SOLID : 0) | (s->dev.medium ? rtk::KEY_MEDIUM : 0) | (s->dev.motion ? rtk::KEY_MOTION : 0) |
                       (s->dev.lens_r != 0.0 ? rtk::KEY_LENS : 0);
  static const std::array<AovKernel, 16> quads_table = aov_quads_kernels(std::make_integer_sequence<int, 16>());
  hipLaunchKernelGGL((s->res->flat.n_quads ? quads_table : table)[features / rtk::KEY_LENS], px_grid(s), dim3(16, 16), 0, (hipStream_t)stream, s->dev, n_samples, (float4*)d_aov);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_hip_denoise(RtHipScene* s, const RtRowTiles* tiles, const void* d_linear, const void* d_aov, uint32_t iterations, float sigma_color,
                              float sigma_normal, float sigma_albedo, float sigma_inv_depth, void* d_out_linear, void* d_out_rgb8, void* stream) {
  int rc = check_whole_frame(s, tiles);
  if (rc != RT_OK) return rc;
  if (iterations > rtc::DENOISE_MAX_ITERATIONS) return fail(RT_ERR_UNSUPPORTED, "at most 8 iterations");
  const float sigma[4] = {sigma_color, sigma_normal, sigma_albedo, sigma_inv_depth};
  if ((rc = check_sigmas(sigma)) != RT_OK) return rc;
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px == 0) return RT_OK;
  if (!d_linear || !d_aov) return fail(RT_ERR_INVALID, "null input buffer");
  if ((rc = check_aligned(d_linear, 4, "d_linear must be 4-byte aligned")) != RT_OK) return rc;
  if ((rc = check_aligned(d_aov, 16, "the AOV buffer must be 16-byte aligned")) != RT_OK) return rc;
  if ((rc = check_aligned(d_out_linear, 4, "d_out_linear must be 4-byte aligned")) != RT_OK) return rc;
  for (const Range out : {Range{d_out_linear, px * 12}, Range{d_out_rgb8, px * 3}})  // (neighbouring threads read the inputs while an output is written)
    if (overlaps(out, {{d_linear, px * 12}, {d_aov, px * 32}})) return fail(RT_ERR_INVALID, "the outputs must not overlap the inputs");
  return denoise_frame(s, d_linear, d_aov, iterations, sigma, d_out_linear, d_out_rgb8, (hipStream_t)stream);
}

extern "C" int rt_hip_refine_to_host_denoised(RtHipScene* s, uint32_t sample_count, uint32_t iterations, uint8_t* out_rgb8, RtStats* stats) {
  if (!s || !out_rgb8) return fail(RT_ERR_INVALID, "null argument");
  if (iterations > rtc::DENOISE_MAX_ITERATIONS) return fail(RT_ERR_UNSUPPORTED, "at most 8 iterations");
  if (s->host.height > 65535u * 16u) return fail(RT_ERR_UNSUPPORTED, "frames taller than 1 048 560 rows");
  return refine_to_host(s, sample_count, (int)iterations, out_rgb8, stats);
}

// ---------------------------------------------------------------------------------------------------- temporal denoising
namespace {
int check_reproject_params(float alpha_min, float n_max, float tau_n, float tau_a, float tau_z) {
  for (float t : {tau_n, tau_a, tau_z})
    if (!(t >= 0.0f) || !(t <= 3.4028234663852886e38f)) return fail(RT_ERR_INVALID, "every threshold must be finite and at least 0");
  if (!(alpha_min >= 0.0f && alpha_min <= 1.0f)) return fail(RT_ERR_INVALID, "alpha_min must lie in [0, 1]");
  if (!(n_max >= 1.0f)) return fail(RT_ERR_INVALID, "n_max must be at least 1");
  return RT_OK;
}
rtc::ReprojCam reproj_cam(const double c[12]) {
  rtc::ReprojCam r;
  for (int i = 0; i < 3; ++i) { r.o[i] = c[i]; r.ll[i] = c[3 + i]; r.h[i] = c[6 + i]; r.v[i] = c[9 + i]; }
  return r;
}
void scene_camera(const RtHipScene* s, double c[12]) {
  for (int i = 0; i < 3; ++i) { c[i] = s->host.cam_origin[i]; c[3 + i] = s->host.cam_lower_left[i]; c[6 + i] = s->host.cam_horizontal[i]; c[9 + i] = s->host.cam_vertical[i]; }
}
// arguments checked by the caller
int reproject_frame(RtHipScene* s, const void* d_linear, const void* d_aov, const void* d_prev_history, const void* d_prev_aov, const double prev_camera[12],
                    const float k[5], void* d_out_history, hipStream_t stream) {
  double cur[12];
  scene_camera(s, cur);
  const rtc::ReprojK rk{k[0], k[1], k[2], k[3], k[4]};
  hipLaunchKernelGGL(rtk::rt_reproject, px_grid(s), dim3(16, 16), 0, stream, (const float*)d_linear, (const float4*)d_aov, (const float4*)d_prev_history,
                     (const float4*)d_prev_aov, reproj_cam(cur), reproj_cam(prev_camera), s->host.width, s->host.height, rk, (float4*)d_out_history);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
}  // namespace

extern "C" int rt_hip_reproject(RtHipScene* s, const void* d_linear, const void* d_aov, const void* d_prev_history, const void* d_prev_aov,
                                const double prev_camera[12], float alpha_min, float n_max, float tau_n, float tau_a, float tau_z, void* d_out_history,
                                void* stream) {
  int rc = check_whole_frame(s, nullptr);
  if (rc != RT_OK) return rc;
  if ((rc = check_reproject_params(alpha_min, n_max, tau_n, tau_a, tau_z)) != RT_OK) return rc;
  if (!d_linear || !d_aov || !d_prev_history || !d_prev_aov || !prev_camera || !d_out_history) return fail(RT_ERR_INVALID, "null argument");
  if ((rc = check_aligned(d_linear, 4, "d_linear must be 4-byte aligned")) != RT_OK) return rc;
  for (const void* q : {d_aov, d_prev_history, d_prev_aov, (const void*)d_out_history})
    if ((rc = check_aligned(q, 16, "the guide and history buffers must be 16-byte aligned")) != RT_OK) return rc;
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px == 0) return RT_OK;
  if (overlaps({d_out_history, px * 16}, {{d_linear, px * 12}, {d_aov, px * 32}, {d_prev_history, px * 16}, {d_prev_aov, px * 32}}))
    return fail(RT_ERR_INVALID, "the output must not overlap the inputs");
  RT_HIP_TRY(hipSetDevice(s->device));
  const float k[5] = {alpha_min, n_max, tau_n, tau_a, tau_z};
  return reproject_frame(s, d_linear, d_aov, d_prev_history, d_prev_aov, prev_camera, k, d_out_history, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------- surface tracking
extern "C" int rt_hip_render_surface(RtHipScene* s, const RtRowTiles* tiles, void* d_surface, void* stream) {
  const int rc = check_whole_frame(s, tiles);
  if (rc != RT_OK) return rc;
  if (!d_surface) return fail(RT_ERR_INVALID, "null surface buffer");
  if (const int refused = check_aligned(d_surface, 16, "the surface buffer must be 16-byte aligned")) return refused;
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px == 0) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  using SurfaceKernel = void (*)(const rtc::DevScene, uint4*);
  static const SurfaceKernel table[8] = {rtk::rt_surface<false, false>, rtk::rt_surface<true, false>, rtk::rt_surface<false, true>, rtk::rt_surface<true, true>,
                                         rtk::rt_surface_quads<false, false>, rtk::rt_surface_quads<true, false>, rtk::rt_surface_quads<false, true>, rtk::rt_surface_quads<true, true>};
  hipLaunchKernelGGL(table[(s->dev.motion ? 1 : 0) | (s->dev.medium ? 2 : 0) | (s->res->flat.n_quads ? 4 : 0)], px_grid(s), dim3(16, 16), 0, (hipStream_t)stream, s->dev, (uint4*)d_surface);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

namespace {
// arguments checked by the caller; k = alpha_min, n_max, tau_n, tau_a, tau_z
int reproject_surface_frame(RtHipScene* s, const void* d_linear, const void* d_aov, const void* d_surface, const void* d_prev_history, const void* d_prev_aov,
                            const void* d_prev_surface, const double prev_camera[12], const double* d_displacement, const float k[5], float alpha_specular,
                            void* d_out_history, hipStream_t stream) {
  double cur[12];
  scene_camera(s, cur);
  rtk::RpSurfArgs a;
  a.lin = (const float*)d_linear; a.aov = (const float4*)d_aov; a.prev_h = (const float4*)d_prev_history; a.prev_aov = (const float4*)d_prev_aov;
  a.surf = (const uint4*)d_surface; a.prev_surf = (const uint4*)d_prev_surface;
  a.disp = d_displacement;
  a.cur = reproj_cam(cur); a.prev = reproj_cam(prev_camera);
  a.n_disp = s->host.n_spheres; a.width = s->host.width; a.height = s->host.height;
  a.k = rtc::ReprojSurfK{k[0], alpha_specular, k[1], k[2], k[3], k[4]};
  hipLaunchKernelGGL(rtk::rt_reproject_surface, px_grid(s), dim3(16, 16), 0, stream, a, (float4*)d_out_history);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
}  // namespace

extern "C" int rt_hip_reproject_surface(RtHipScene* s, const void* d_linear, const void* d_aov, const void* d_surface, const void* d_prev_history,
                                        const void* d_prev_aov, const void* d_prev_surface, const double prev_camera[12], const double* d_displacement,
                                        float alpha_min, float alpha_specular, float n_max, float tau_n, float tau_a, float tau_z, void* d_out_history,
                                        void* stream) {
  int rc = check_whole_frame(s, nullptr);
  if (rc != RT_OK) return rc;
  if ((rc = check_reproject_params(alpha_min, n_max, tau_n, tau_a, tau_z)) != RT_OK) return rc;
  if (!(alpha_specular >= 0.0f && alpha_specular <= 1.0f)) return fail(RT_ERR_INVALID, "alpha_specular must lie in [0, 1]");
  if (!d_linear || !d_aov || !d_surface || !d_prev_history || !d_prev_aov || !d_prev_surface || !prev_camera || !d_out_history)
    return fail(RT_ERR_INVALID, "null argument");
  if ((rc = check_aligned(d_linear, 4, "d_linear must be 4-byte aligned")) != RT_OK) return rc;
  for (const void* q : {d_aov, d_surface, d_prev_history, d_prev_aov, d_prev_surface, (const void*)d_out_history})
    if ((rc = check_aligned(q, 16, "the guide, surface and history buffers must be 16-byte aligned")) != RT_OK) return rc;
  if ((rc = check_aligned(d_displacement, 8, "the displacement table must be 8-byte aligned")) != RT_OK) return rc;
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px == 0) return RT_OK;
  if (overlaps({d_out_history, px * 16}, {{d_linear, px * 12}, {d_aov, px * 32}, {d_surface, px * 16}, {d_prev_history, px * 16}, {d_prev_aov, px * 32},
                                          {d_prev_surface, px * 16}, {d_displacement, d_displacement ? (size_t)s->host.n_spheres * 24 : (size_t)0}}))
    return fail(RT_ERR_INVALID, "the output must not overlap the inputs");
  RT_HIP_TRY(hipSetDevice(s->device));
  const float k[5] = {alpha_min, n_max, tau_n, tau_a, tau_z};
  return reproject_surface_frame(s, d_linear, d_aov, d_surface, d_prev_history, d_prev_aov, d_prev_surface, prev_camera, d_displacement, k, alpha_specular,
                                 d_out_history, (hipStream_t)stream);
}

extern "C" int rt_hip_temporal_configure(RtHipScene* s, float alpha_min, float n_max, float tau_n, float tau_a, float tau_z) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  const int rc = check_reproject_params(alpha_min, n_max, tau_n, tau_a, tau_z);
  if (rc != RT_OK) return rc;
  const float k[5] = {alpha_min, n_max, tau_n, tau_a, tau_z};
  std::memcpy(s->tp.k, k, sizeof k);
  return RT_OK;
}

extern "C" int rt_hip_temporal_reset(RtHipScene* s) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  RT_HIP_TRY(hipSetDevice(s->device));
  if (s->n_launches) RT_HIP_TRY(hipStreamSynchronize(s->last_stream));  // (the host form is blocking: nothing of it is in flight; a caller's own launch may be)
  s->tp.reset();
  return RT_OK;
}

// Surface tracking on or off for the host form; a real change drops the history.
extern "C" int rt_hip_temporal_surface(RtHipScene* s, int enable, float alpha_specular) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  if (!(alpha_specular >= 0.0f && alpha_specular <= 1.0f)) return fail(RT_ERR_INVALID, "alpha_specular must lie in [0, 1]");
  const bool on = enable != 0;
  if (on != s->tp.surface) {
    const int rc = rt_hip_temporal_reset(s);
    if (rc != RT_OK) return rc;
    s->tp.surface = on;
  }
  s->tp.alpha_specular = alpha_specular;
  return RT_OK;
}

extern "C" int rt_hip_temporal_history(RtHipScene* s, float* out_history) {
  if (!s || !out_history) return fail(RT_ERR_INVALID, "null argument");
  if (!s->tp.valid) return fail(RT_ERR_INVALID, "the scene holds no temporal history");
  RT_HIP_TRY(hipSetDevice(s->device));
  const size_t px = (size_t)s->host.width * s->host.height;
  if (px) RT_HIP_TRY(hipMemcpy(out_history, s->tp.hist[s->tp.cur].p, px * 16, hipMemcpyDeviceToHost));
  return RT_OK;
}

// One frame of an animation, blocking, on the NULL stream like rt_hip_render_to_host: samples [b, b + spp) into the frame's own
// accumulator, resolved to linear f32, the AOVs of this view, one reprojection step against the history the previous call left, and
// the spatial filter over the new history's rgb into RGB8.  The history keeps the colour BEFORE the filter.
extern "C" int rt_hip_render_frame_temporal_to_host(RtHipScene* s, uint32_t frame_index, uint32_t iterations, uint8_t* out_rgb8, RtStats* stats) {
  if (!s || !out_rgb8) return fail(RT_ERR_INVALID, "null argument");
  if (iterations > rtc::DENOISE_MAX_ITERATIONS) return fail(RT_ERR_UNSUPPORTED, "at most 8 iterations");
  int rc = check_whole_frame(s, nullptr);
  if (rc != RT_OK) return rc;
  const uint32_t spp = s->host.samples_per_pixel;
  if (spp == 0) return fail(RT_ERR_INVALID, "samples_per_pixel must be at least 1");
  if ((rc = check_samples(0, spp)) != RT_OK) return rc;
  const uint32_t F = rtc::ACCUM_MAX_SAMPLES / spp, begin = (frame_index % F) * spp;  // (frames F apart share a sample range)
  HostForm f{s};
  if ((rc = f.begin()) != RT_OK) return rc;
  const size_t px = (size_t)s->host.width * s->host.height, bytes = px * 3;
  bool grew = false, any_grew = false;
  if ((rc = s->tp.accum.ensure(px * 24)) != RT_OK || (rc = s->prog.dn_lin.ensure(px * 12)) != RT_OK || (rc = s->frame.ensure(bytes)) != RT_OK) return rc;
  for (int i = 0; i < 2; ++i) {
    if ((rc = s->tp.hist[i].ensure(px * 16, &grew)) != RT_OK) return rc;
    any_grew = any_grew || grew;
    if ((rc = s->tp.aov[i].ensure(px * 32, &grew)) != RT_OK) return rc;
    any_grew = any_grew || grew;
  }
  const uint32_t n_sph = s->host.n_spheres;
  if (s->tp.surface) {
    for (int i = 0; i < 2; ++i) {
      if ((rc = s->tp.surf[i].ensure(px * 16, &grew)) != RT_OK) return rc;
      any_grew = any_grew || grew;
    }
    if ((rc = s->tp.disp.ensure(n_sph ? (size_t)n_sph * 24 : 16)) != RT_OK) return rc;
  }
  if (any_grew) s->tp.valid = false;
  const int prev = s->tp.cur, cur = prev ^ 1;
  double prev_cam[12];
  if (s->tp.valid) std::memcpy(prev_cam, s->tp.cam, sizeof prev_cam);
  else {  // no previous frame: a history of n = 0 everywhere, which no tap accepts
    scene_camera(s, prev_cam);
    if (px) {
      RT_HIP_TRY(hipMemsetAsync(s->tp.hist[prev].p, 0, px * 16, nullptr));
      RT_HIP_TRY(hipMemsetAsync(s->tp.aov[prev].p, 0, px * 32, nullptr));
      if (s->tp.surface) RT_HIP_TRY(hipMemsetAsync(s->tp.surf[prev].p, 0, px * 16, nullptr));
    }
  }
  if (s->tp.surface && n_sph) {  // each sphere's centre now minus its centre in the tables the previous temporal frame rendered with
    const std::vector<double>& now = s->res->sph.mid;
    const bool have = s->tp.valid && s->tp.mid.size() == now.size();
    s->tp.disp_host.resize(now.size());
    for (size_t i = 0; i < now.size(); ++i) s->tp.disp_host[i] = have ? now[i] - s->tp.mid[i] : 0.0;
    RT_HIP_TRY(hipMemcpy(s->tp.disp.p, s->tp.disp_host.data(), (size_t)n_sph * 24, hipMemcpyHostToDevice));
  }
  if (px) RT_HIP_TRY(hipMemsetAsync(s->tp.accum.p, 0, px * 24, nullptr));
  rc = rt_hip_accumulate(s, nullptr, begin, spp, s->tp.accum.p, nullptr);
  if (rc == RT_OK) rc = rt_hip_resolve(s, nullptr, s->tp.accum.p, spp, nullptr, s->prog.dn_lin.p, nullptr);
  if (rc == RT_OK) rc = rt_hip_render_aovs(s, nullptr, aov_default_samples(spp), s->tp.aov[cur].p, nullptr);
  if (s->tp.surface) {
    if (rc == RT_OK) rc = rt_hip_render_surface(s, nullptr, s->tp.surf[cur].p, nullptr);
    if (rc == RT_OK && px)
      rc = reproject_surface_frame(s, s->prog.dn_lin.p, s->tp.aov[cur].p, s->tp.surf[cur].p, s->tp.hist[prev].p, s->tp.aov[prev].p, s->tp.surf[prev].p, prev_cam,
                                   n_sph ? s->tp.disp.get<const double>() : nullptr, s->tp.k, s->tp.alpha_specular, s->tp.hist[cur].p, nullptr);
  } else
  if (rc == RT_OK && px) rc = reproject_frame(s, s->prog.dn_lin.p, s->tp.aov[cur].p, s->tp.hist[prev].p, s->tp.aov[prev].p, prev_cam, s->tp.k, s->tp.hist[cur].p, nullptr);
  const float sigma[4] = {RT_DENOISE_SIGMA_COLOR, RT_DENOISE_SIGMA_NORMAL, RT_DENOISE_SIGMA_ALBEDO, RT_DENOISE_SIGMA_INV_DEPTH};
  if (rc == RT_OK) rc = denoise_frame(s, s->tp.hist[cur].p, s->tp.aov[cur].p, iterations, sigma, nullptr, s->frame.p, nullptr, true);
  if ((rc = f.wait(rc)) != RT_OK) { s->tp.valid = false; return rc; }  // (a frame that did not complete leaves the history unknown: start over)
  if ((rc = f.deliver(out_rgb8, stats)) != RT_OK) return rc;
  s->tp.cur = cur;
  s->tp.valid = true;
  scene_camera(s, s->tp.cam);
  if (s->tp.surface) s->tp.mid = s->res->sph.mid;
  return RT_OK;
}

// Adaptive sampling, host form, blocking, on the NULL stream like rt_hip_render_to_host.  M = min(min_spp, N):
// round 0 renders [0, M/2) and [M/2, M) into every tile with a snapshot between them; after a round that brought its tiles to n,
// a tile goes on iff n < N and its error >= threshold, and the next round adds min(n, N - n) samples to every tile that goes on.
// Every pixel is the one-shot frame at its tile's count.  M < 2: the one-shot frame.
extern "C" int rt_hip_render_adaptive_to_host(RtHipScene* s, double threshold, uint32_t min_spp, uint8_t* out_rgb8, uint32_t* out_tile_spp,
                                              RtStats* stats) {
  if (!s || !out_rgb8) return fail(RT_ERR_INVALID, "null argument");
  if (!(threshold >= 0.0) || std::isinf(threshold)) return fail(RT_ERR_INVALID, "the threshold must be finite and at least 0");
  if (min_spp == 0) return fail(RT_ERR_INVALID, "min_spp must be at least 1");
  const uint32_t N = s->host.samples_per_pixel;
  if (const int refused = check_samples(0, N, "an adaptive frame holds ")) return refused;
  HostForm f{s};  // (its clock and the device: the frame's stats are summed over the rounds below)
  int rc = f.begin();
  if (rc != RT_OK) return rc;
  TileGeom tg;
  if ((rc = tile_geometry(s, s->host.height, &tg)) != RT_OK) return rc;
  const uint32_t nt = tg.tiles_x * tg.tiles_y, M = min_spp < N ? min_spp : N;
  s->ad.reset();
  if (M < 2) {  // (no estimate can be made: every tile at N)
    RtStats st;
    if ((rc = rt_hip_render_to_host(s, out_rgb8, &st)) != RT_OK) return rc;
    s->ad.rounds.push_back({nt, N, st.kernel_ms});
    if (out_tile_spp) std::fill(out_tile_spp, out_tile_spp + nt, N);
    if (stats) { *stats = st; stats->frame_ms = f.ms(); }
    return RT_OK;
  }
  const size_t px = (size_t)s->host.width * s->host.height, bytes = px * 24;
  if ((rc = s->ad.now.ensure(bytes)) != RT_OK || (rc = s->ad.prev.ensure(bytes)) != RT_OK || (rc = s->ad.list.ensure((size_t)nt * 4)) != RT_OK ||
      (rc = s->ad.err.ensure((size_t)nt * 8)) != RT_OK || (rc = s->ad.spp.ensure((size_t)nt * 4)) != RT_OK || (rc = s->frame.ensure(px * 3)) != RT_OK)
    return rc;
  unsigned long long* const now = s->ad.now.get<unsigned long long>(), * const prev = s->ad.prev.get<unsigned long long>();
  uint32_t* const d_list = s->ad.list.get<uint32_t>();
  RtStats total;
  std::memset(&total, 0, sizeof total);
  total.n_gpus_used = 1;
  double round_ms = 0.0;
  auto collect = [&]() -> int {  // the launch just enqueued: wait for it, add its figures to the frame's
    RtStats st;
    const int rc = rt_hip_wait(s, &st);
    if (rc != RT_OK) return rc;
    total.segments += st.segments; total.sphere_tests += st.sphere_tests; total.exact_tests += st.exact_tests;
    total.tex_oob += st.tex_oob; total.grid_steps += st.grid_steps;
    for (int k = 0; k < 4; ++k) total.wave_iters[k] += st.wave_iters[k];
    for (int k = 0; k < 12; ++k) total.prof_cycles[k] += st.prof_cycles[k];
    const uint64_t rep = (uint64_t)total.segments_repeated + st.segments_repeated;
    total.segments_repeated = rep > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rep;
    total.kernel_ms += st.kernel_ms; round_ms += st.kernel_ms;
    return RT_OK;
  };
  std::vector<uint32_t> n_t(nt, M), list(nt);
  std::vector<double> err(nt, 0.0);
  for (uint32_t t = 0; t < nt; ++t) list[t] = nt - 1u - t;  // (bottom of the image first, the kernel's own default order)
  // round 0: every tile, two halves, the estimate between them
  const uint32_t h = M / 2u;
  RT_HIP_TRY(hipMemsetAsync(now, 0, bytes, nullptr));
  if ((rc = rt_hip_accumulate(s, nullptr, 0u, h, now, nullptr)) != RT_OK || (rc = collect()) != RT_OK) return rc;
  RT_HIP_TRY(hipMemcpyAsync(prev, now, bytes, hipMemcpyDeviceToDevice, nullptr));
  if ((rc = rt_hip_accumulate(s, nullptr, h, M - h, now, nullptr)) != RT_OK || (rc = collect()) != RT_OK) return rc;
  RT_HIP_TRY(hipMemcpy(d_list, list.data(), (size_t)nt * 4, hipMemcpyHostToDevice));
  uint32_t n = M, n_prev = h;
  s->ad.rounds.push_back({nt, n, round_ms});
  for (;;) {
    if (n >= N) break;
    if ((rc = rt_hip_tile_error(s, nullptr, d_list, (uint32_t)list.size(), now, n, prev, n_prev, s->ad.err.get<double>(), nullptr)) != RT_OK) return rc;
    RT_HIP_TRY(hipMemcpy(err.data(), s->ad.err.get<double>(), (size_t)nt * 8, hipMemcpyDeviceToHost));
    size_t k = 0;
    for (uint32_t t : list) if (err[t] >= threshold) list[k++] = t;
    list.resize(k);
    if (list.empty()) break;
    const uint32_t add = n < N - n ? n : N - n;
    round_ms = 0.0;
    RT_HIP_TRY(hipMemcpyAsync(prev, now, bytes, hipMemcpyDeviceToDevice, nullptr));
    RT_HIP_TRY(hipMemcpy(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    if ((rc = rt_hip_accumulate_tiles(s, nullptr, d_list, (uint32_t)list.size(), n, add, now, nullptr)) != RT_OK || (rc = collect()) != RT_OK)
      return rc;
    n_prev = n; n += add;
    for (uint32_t t : list) n_t[t] = n;
    s->ad.rounds.push_back({(uint32_t)list.size(), n, round_ms});
  }
  RT_HIP_TRY(hipMemcpy(s->ad.spp.get<uint32_t>(), n_t.data(), (size_t)nt * 4, hipMemcpyHostToDevice));
  if ((rc = rt_hip_resolve_tiles(s, nullptr, now, s->ad.spp.get<uint32_t>(), s->frame.p, nullptr, nullptr)) != RT_OK) return rc;
  RT_HIP_TRY(hipMemcpy(out_rgb8, s->frame.p, px * 3, hipMemcpyDeviceToHost));
  if (out_tile_spp) std::copy(n_t.begin(), n_t.end(), out_tile_spp);
  if (stats) {
    uint64_t samples = 0;
    const uint32_t tw = 1u << tg.tile_wl, th = 1u << tg.tile_hl;
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t by = t / tg.tiles_x, bx = t - by * tg.tiles_x;
      const uint64_t w = std::min<uint64_t>(tw, s->host.width - bx * tw), hh = std::min<uint64_t>(th, s->host.height - by * th);
      samples += w * hh * n_t[t];
    }
    total.samples = samples;
    total.frame_ms = f.ms();
    *stats = total;
  }
  return RT_OK;
}

// The scene's own kernel through the stream its frames will use, once, on ONE scanline — whatever the runtime does with the first
// launch of a kernel on a queue (its scratch, its kernarg pool, the instruction cache) happens here, at set-up, instead of inside
// the first frame: the group calls it per rank.  The launch leaves no trace in the scene (slots, queue order, counters of the
// "last launch" are as after creation).
int rt_hip_scene_warm(RtHipScene* s, hipStream_t stream) {
  if (!s || s->host.width == 0 || s->host.height == 0) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  DevBuf row;
  int rc = row.ensure((size_t)s->host.width * 3 + 16);
  if (rc != RT_OK) return rc;
  const int saved_order = s->opt.order_mode;
  s->opt.order_mode = 1;  // (nothing measured, nothing sorted)
  const RtRowTiles first_row{1u, 0u, s->host.height};
  rc = rt_hip_render(s, &first_row, row.p, nullptr, stream);
  RtStats wst;
  if (rc == RT_OK) rc = rt_hip_wait(s, &wst);
  if (rc == RT_OK) rtp::add("rank0.warm_up_kernel_ms_by_events", wst.kernel_ms);
  s->opt.order_mode = saved_order;
  s->n_launches = 0; s->in_flight = false; s->last_stream = nullptr; s->last_waves = 0;
  s->order.key = RtHipScene::OrderKey(); s->order.forget();
  for (auto& sl : s->slot) { sl.rows = 0; sl.samples = 0; sl.waves = 0; sl.launched = false; }
  return rc;
}


// ------------------------------------------------------------------------------ moving the spheres of a resident scene
namespace {
// Point a scene (or a view) at its resident's live tables and start over what was derived from the old ones: the launch
// configuration (as creation derives it), the learned tile order, the progressive accumulator with its cached AOVs, the adaptive rounds;
// and where the flat primitives moved, the temporal history (rt_hip_reproject_surface takes a flat id as "not displaced": a moved flat
// primitive is not followed through the filter)
int adopt_tables(RtHipScene* s, Moved what) {
  if (what == Moved::flats) s->tp.reset();
  s->res->point(s->dev);
  s->order.forget();
  s->prog.reset();
  s->ad.reset();
  return configure(s);
}

// an update of a scene replaces tables its views read: only a caller that re-points them itself (views_follow: the group) may run it while
// there is a view.  who, through, group_call: the entry point, the message's verb, the group's call of the same name
int check_not_shared(const RtHipScene* s, bool views_follow, const char* who, const char* through, const char* group_call) {
  if (views_follow || s->res.use_count() <= 1) return RT_OK;
  return fail(RT_ERR_INVALID, std::string(who) + ": the scene's tables are shared with a view (a group " + through + " " + group_call + ")");
}

// views_follow: the caller (the group) re-points the views that share this scene's tables itself
int scene_update(RtHipScene* s, const double* center, const double* center1, bool views_follow) {
  if (!s || (!center && s->host.n_spheres)) return fail(RT_ERR_INVALID, "null argument");
  if (const int refused = check_not_shared(s, views_follow, "rt_hip_scene_update_spheres", "updates through", "rt_hip_group_update_spheres")) return refused;
  int rc;
  if ((rc = make_current_and_drain(s)) != RT_OK) return rc;
  rtp::Clock pc = rtp::begin();
  RtHipScene::Resident::Spheres& r = s->res->sph;
  const uint32_t n = s->host.n_spheres;
  // the host's part: the spheres at their new centres, the motion rows, the plan of the grid (rt_tables.h: creation's own code)
  std::vector<RtSphere>& next = r.next_spheres;
  if (next.size() != r.spheres.size()) next = r.spheres;
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) next[i].center[k] = center[3 * (size_t)i + k];
  RtScene sc = s->host;
  sc.spheres = next.data();
  rtc::HostTables t;
  const std::string why = rtc::build_motion(sc, center1, t);
  if (!why.empty()) return fail(RT_ERR_INVALID, why);
  const rtc::GridParams gp = rtc::grid_params_shipped();
  const bool want_wide = gp.force_wide || n > 65535u;
  rtgb::Job j;
  rtc::GridPlan& plan = r.plan;
  j.all_large = rtc::grid_plan(sc, t, gp, want_wide, j.G, plan) != rtc::GRID_PLAN_GRID;
  if (j.all_large) std::memset(&j.G, 0, sizeof j.G);
  pc.mark("update.host_plan");
  const uint32_t inner = j.all_large ? 0u : rtgb::inner_cells(j.G);
  RtHipScene::Resident::Spheres::Scratch& gb = r.scratch;
  RtHipScene::Resident::Spheres::Tables& spare = r.spare;
  if ((rc = room(gb.centre, (size_t)n * 24)) != RT_OK || (rc = room(gb.plan_large, n)) != RT_OK || (rc = room(gb.range, (size_t)n * sizeof(rtc::GridRange))) != RT_OK ||
      (rc = room(gb.lflag, (size_t)n * 4)) != RT_OK || (rc = room(gb.lpos, (size_t)n * 4)) != RT_OK || (rc = room(gb.count, (size_t)inner * 4)) != RT_OK ||
      (rc = room(gb.start, (size_t)inner * 4)) != RT_OK || (rc = room(gb.cursor, (size_t)inner * 4)) != RT_OK ||
      (rc = room(gb.block_sum, (rtgb::scan_blocks(std::max<size_t>(n, inner)) + 1) * 8)) != RT_OK || (rc = room(gb.counts, sizeof(rtgb::Counts))) != RT_OK ||
      (rc = room(spare.geom, (size_t)n * sizeof(rtc::SphereGeom))) != RT_OK || (t.n_moving && (rc = room(spare.motion, (size_t)n * 32)) != RT_OK))
    return rc;
  if (n) RT_HIP_TRY(hipMemcpy(gb.centre.p, center, (size_t)n * 24, hipMemcpyHostToDevice));  // (the centres travel once)
  if (!j.all_large) RT_HIP_TRY(hipMemcpy(gb.plan_large.p, plan.is_large.data(), n, hipMemcpyHostToDevice));
  if (t.n_moving) {  // (uploaded from storage that lives as long as the scene)
    r.keep_motion.assign(t.motion.begin(), t.motion.end());
    RT_HIP_TRY(hipMemcpy(spare.motion.p, r.keep_motion.data(), (size_t)n * 32, hipMemcpyHostToDevice));
  }
  pc.mark("update.upload");
  j.n = n;
  for (int k = 0; k < 3; ++k) j.cell_w[k] = plan.cell_w[k];
  j.m = plan.m; j.large_cell_limit = gp.large_cell_limit;
  j.centre = gb.centre.get<const double>(); j.old_geom = r.live.geom.get<const rtc::SphereGeom>();
  j.motion = t.n_moving ? spare.motion.get<const double>() : nullptr;
  j.plan_large = gb.plan_large.get<const uint8_t>();
  j.range = gb.range.get<rtc::GridRange>(); j.lflag = gb.lflag.get<uint32_t>(); j.lpos = gb.lpos.get<uint32_t>();
  j.count = gb.count.get<uint32_t>(); j.start = gb.start.get<uint32_t>(); j.cursor = gb.cursor.get<uint32_t>();
  j.block_sum = gb.block_sum.get<unsigned long long>(); j.counts = gb.counts.get<rtgb::Counts>();
  j.geom = spare.geom.get<rtc::SphereGeom>();
  rtgb::Counts cnt;
  RT_HIP_TRY(rtgb::count(j, nullptr));
  RT_HIP_TRY(hipMemcpy(&cnt, gb.counts.p, sizeof cnt, hipMemcpyDeviceToHost));  // the one readback: item total, fullest cell, `large` count
  bool wide = want_wide;
  if (!j.all_large && cnt.n_items >= 0xFFFFFFFEull) {  // (more items than a 32-bit list holds: no grid, as build_grid_as decides)
    j.all_large = true;
    std::memset(&j.G, 0, sizeof j.G);
    RT_HIP_TRY(rtgb::count(j, nullptr));
    RT_HIP_TRY(hipMemcpy(&cnt, gb.counts.p, sizeof cnt, hipMemcpyDeviceToHost));
  }
  // the packed format's limits, where build_grid falls back to the wide one
  if (!j.all_large && !wide && (cnt.max_count > rtc::CELL_MAX_COUNT || cnt.n_items >= rtc::CELL_START_MASK)) wide = true;
  pc.mark("update.count_kernels_and_readback");
  j.G.n_items = (uint32_t)cnt.n_items; j.G.n_large = (uint32_t)cnt.n_large; j.G.wide = (!j.all_large && wide) ? 1u : 0u;
  if ((rc = check_wide_tables(j.G.wide, s->res->n_media, s->res->n_solids, s->res->flat.n_quads != 0)) != RT_OK) return rc;
  if ((rc = room(spare.cell_word, (size_t)j.G.n_cells * (j.G.wide ? 16u : 8u))) != RT_OK || (rc = room(spare.cell_items, (size_t)j.G.n_items * (j.G.wide ? 4u : 2u))) != RT_OK ||
      (rc = room(gb.raw_items, (size_t)j.G.n_items * 4)) != RT_OK || (rc = room(gb.raw_cell, (size_t)j.G.n_items * 4)) != RT_OK ||
      (rc = room(spare.large, (size_t)j.G.n_large * 4)) != RT_OK || (rc = room(spare.large_geom, (size_t)j.G.n_large * sizeof(rtc::SphereGeom))) != RT_OK)
    return rc;
  j.raw_items = gb.raw_items.get<uint32_t>(); j.raw_cell = gb.raw_cell.get<uint32_t>();
  j.cell_word = spare.cell_word.get<uint32_t>(); j.cell_items = spare.cell_items.p;
  j.large = spare.large.get<uint32_t>(); j.large_geom = spare.large_geom.get<rtc::SphereGeom>();
  RT_HIP_TRY(rtgb::tables(j, cnt.n_items, cnt.n_large, j.G.wide != 0u, nullptr));
  RT_HIP_TRY(hipDeviceSynchronize());
  pc.mark("update.table_kernels");
  // every table is built: swap the generation in (nothing above changed what the scene renders with)
  spare.n_moving = t.n_moving;
  spare.grid = j.G;
  std::swap(r.live, spare);  // (the motion buffers change hands too, moving tables or not: Tables::motion)
  r.spheres.swap(r.next_spheres);
  r.set_mid(t.motion);
  rc = adopt_tables(s, Moved::spheres);
  pc.mark("update.configuration");
  return rc;
}
}  // namespace

// a view follows its scene's update (internal; rt_hip_group_update_spheres, rt_hip_group_update_flats): the tables it shares have been replaced
int rt_hip_scene_view_follow(RtHipScene* view, Moved what) {
  if (!view) return fail(RT_ERR_INVALID, "null argument");
  if (const int rc = make_current_and_drain(view)) return rc;
  return adopt_tables(view, what);
}

extern "C" int rt_hip_scene_update_spheres(RtHipScene* s, const double* center, const double* center1) {
  return scene_update(s, center, center1, false);
}

#include "rt_hip_flats.hip"  // rt_hip_scene_update_flats and rt_hip_scene_set_flat_*: changing the flat primitives of a resident scene

// diagnostics: one resident table as the kernels read it
extern "C" int rt_hip_scene_table(const RtHipScene* s, const char* name, void* out, size_t cap, size_t* needed) {
  if (!s || !name) return fail(RT_ERR_INVALID, "null argument");
  const RtHipScene::Resident::Spheres::Tables& r = s->res->sph.live;
  const RtHipScene::Resident::Flats& f = s->res->flat;
  const rtc::GridDesc& G = r.grid;
  const void* src = nullptr;
  size_t bytes = 0;
  bool host = false;
  if (!std::strcmp(name, "grid")) { src = &G; bytes = sizeof G; host = true; }
  else if (!std::strcmp(name, "cell_word")) { src = r.cell_word.p; bytes = (size_t)G.n_cells * (G.wide ? 16u : 8u); }
  else if (!std::strcmp(name, "cell_items")) { src = r.cell_items.p; bytes = (size_t)G.n_items * (G.wide ? 4u : 2u); }
  else if (!std::strcmp(name, "large")) { src = r.large.p; bytes = (size_t)G.n_large * 4; }
  else if (!std::strcmp(name, "geom")) { src = r.geom.p; bytes = (size_t)s->host.n_spheres * sizeof(rtc::SphereGeom); }
  else if (!std::strcmp(name, "large_geom")) { src = r.large_geom.p; bytes = (size_t)G.n_large * sizeof(rtc::SphereGeom); }
  else if (!std::strcmp(name, "motion")) { src = r.n_moving ? r.motion.p : nullptr; bytes = r.n_moving ? (size_t)s->host.n_spheres * 32 : 0; }
  else if (!std::strcmp(name, "quads")) { src = f.first_rec(f.live); bytes = (size_t)f.n_quads * sizeof(RtQuadRec); }
  else if (!std::strcmp(name, "quad_lim")) { src = f.lim.p; bytes = f.n_tris ? (size_t)f.n_quads * sizeof(double) : 0; }
  else if (!std::strcmp(name, "flat_bvh")) { src = f.live.nodes.p; bytes = (size_t)f.n_nodes * sizeof(rtc::FlatNode); }
  else if (!std::strcmp(name, "flat_motion")) { src = f.motion.p; bytes = f.n_moving ? (size_t)f.n_quads * 32u : 0; }
  else if (!std::strcmp(name, "flat_normals")) { src = f.normals.p; bytes = f.n_normals ? (size_t)f.n_quads * 72u : 0; }
  else if (!std::strcmp(name, "flat_images")) { src = f.images.p; bytes = f.n_images ? (size_t)f.n_quads * sizeof(RtFlatImageRec) : 0; }
  else if (!std::strcmp(name, "flat_lights")) { src = s->res->flat_lights.data(); bytes = s->res->flat_lights.size() * sizeof(uint32_t); host = true; }  // (§28: the emitters' entry indices in light order)
  else if (!std::strcmp(name, "lights")) { src = s->res->lights.p; bytes = (size_t)s->res->n_lights() * sizeof(uint32_t); }
  else if (!std::strcmp(name, "mat")) { src = s->res->mat.p; bytes = ((size_t)s->host.n_spheres + f.n_quads) * sizeof(rtc::SphereMat); }
  else if (!std::strcmp(name, "matc")) { src = s->res->matc.p; bytes = ((size_t)s->host.n_spheres + f.n_quads) * sizeof(rtc::MatCore); }
  else if (!std::strcmp(name, "flat_bvh_order")) { src = f.live.order.p; bytes = f.n_nodes ? (size_t)f.n_quads * sizeof(uint32_t) : 0; }
  else return fail(RT_ERR_INVALID, std::string("unknown table ") + name);
  if (needed) *needed = bytes;
  if (!out) return RT_OK;
  if (cap < bytes) return fail(RT_ERR_INVALID, "the buffer is smaller than the table");
  if (!bytes) return RT_OK;
  if (host) { std::memcpy(out, src, bytes); return RT_OK; }
  RT_HIP_TRY(hipSetDevice(s->device));
  RT_HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

#include "rt_hip_group.hip"  // rt_hip_group_* and rt_render_rgb8: the frame over 1..G devices

#ifdef RT_TEST_PROBES
// math self-test hook (see rtk::rt_math_probe); all pointers are DEVICE pointers
extern "C" int rt_hip_hit_probe(const double* rays, const double* spheres, double* out_t, uint32_t n, void* stream) {
  hipLaunchKernelGGL(rtk::rt_hit_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rays, spheres, out_t, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_hip_math_probe(const double* x, const double* y, double* out_sqrt, double* out_div, float* out_sqrtf,
                                 double* out_atan2, uint32_t n, void* stream) {
  hipLaunchKernelGGL(rtk::rt_math_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y, out_sqrt, out_div,
                     out_sqrtf, out_atan2, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_hip_atan2_probe(const double* d_y, const double* d_x, double* d_out, uint32_t n, void* stream) {
  if (!d_y || !d_x || !d_out) return fail(RT_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(rtk::rt_atan2_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_y, d_x, d_out, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// device probe of the Texture hit's fast texel path beside the exact one (see rtk::rt_texel_probe); d_* are DEVICE pointers
extern "C" int rt_hip_texel_probe(const double* d_points, const double centre_radius[4], double h_offset, uint64_t tex_w, uint64_t tex_h,
                                  uint64_t* d_out, double* d_uv, uint32_t n, void* stream) {
  if (!d_points || !centre_radius || !d_out) return fail(RT_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(rtk::rt_texel_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_points, centre_radius[0], centre_radius[1],
                     centre_radius[2], centre_radius[3], h_offset, (unsigned long long)tex_w, (unsigned long long)tex_h,
                     (unsigned long long*)d_out, d_uv, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// a frame of the scene's own launch path whose camera rays are the caller's (see rtk::KArgs.probe_rays); d_* are DEVICE pointers
extern "C" int rt_hip_render_rays_probe(RtHipScene* s, const double* d_rays, double* d_first_t, int32_t* d_first_sphere, void* d_rgb8,
                                        void* d_linear, RtStats* stats) {
  if (!s || !d_rays || !d_rgb8) return fail(RT_ERR_INVALID, "null argument");
  if (!d_first_t != !d_first_sphere) return fail(RT_ERR_INVALID, "the first-hit record needs both d_first_t and d_first_sphere");
  if (s->host.samples_per_pixel > (1u << 22)) return fail(RT_ERR_UNSUPPORTED, "more than 2^22 samples per pixel");
  g_probe_rays.rays = d_rays; g_probe_rays.t = d_first_t; g_probe_rays.best = d_first_sphere;
  int rc = launch_frame(s, nullptr, d_rgb8, d_linear, nullptr, 0u, s->host.samples_per_pixel, nullptr);
  g_probe_rays = ProbeRays();
  if (rc == RT_OK) rc = rt_hip_wait(s, stats);
  return rc;
}

// rt_core.h hit_world_grid of n rays on the device, one per thread, through the scene's tables (see rtk::rt_walk_probe)
extern "C" int rt_hip_walk_probe(RtHipScene* s, const double* d_rays, double* d_t, int32_t* d_best, uint32_t* d_work, uint32_t n, void* stream) {
  if (!s || !d_rays || !d_t || !d_best) return fail(RT_ERR_INVALID, "null argument");
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_walk_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->dev, d_rays, d_t, d_best, d_work, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// rt_core.h quads_hit / object_surface<true> of n rays on the device, one per thread, against a range of the scene's quads (see
// rtk::rt_quad_probe)
extern "C" int rt_hip_quad_probe(RtHipScene* s, const double* d_rays, const double* d_closest, uint32_t n, uint32_t first_quad, uint32_t n_quads,
                                 int32_t* d_best, double* d_t, double* d_point, double* d_normal, int32_t* d_front, void* stream) {
  if (!s || !d_rays || !d_closest || !d_best || !d_t || !d_point || !d_normal || !d_front) return fail(RT_ERR_INVALID, "null argument");
  if (first_quad > s->res->flat.n_quads || n_quads > s->res->flat.n_quads - first_quad) return fail(RT_ERR_INVALID, "the range lies outside the scene's quads");
  if (!n) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_quad_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->dev, d_rays, d_closest, n, first_quad, n_quads,
                     d_best, d_t, d_point, d_normal, d_front);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_hip_quot_probe(const double* d_x, const double* d_y, double* d_quot, double* d_rsqrt, double* d_div, uint32_t n, void* stream) {
  if (!d_x || !d_y || !d_quot || !d_rsqrt) return fail(RT_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(rtk::rt_quot_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_x, d_y, d_quot, d_rsqrt, d_div, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// csrc/common/rt_neg_log.h and rt_solid.h as the device evaluates them (see rtk::rt_neg_log_probe, rtk::rt_solid_fn_probe)
extern "C" int rt_hip_neg_log_probe(const double* d_x, double* d_out, uint32_t n, void* stream) {
  if (!d_x || !d_out) return fail(RT_ERR_INVALID, "null argument");
  if (!n) return RT_OK;
  hipLaunchKernelGGL(rtk::rt_neg_log_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_x, d_out, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
extern "C" int rt_hip_solid_fn_probe(const double* d_p, uint32_t mode, uint32_t octaves, uint32_t seed, double* d_noise, double* d_factor,
                                     int32_t* d_checker_odd, uint32_t n, void* stream) {
  if (!d_p) return fail(RT_ERR_INVALID, "null argument");
  if (mode > RT_SOLID_MODE_MARBLE || octaves < 1u || octaves > RT_SOLID_MAX_OCTAVES) return fail(RT_ERR_INVALID, "mode 0..2 and 1..16 octaves");
  if (!n) return RT_OK;
  hipLaunchKernelGGL(rtk::rt_solid_fn_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_p, mode, octaves, seed, d_noise, d_factor,
                     d_checker_odd, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// rt_core.h solid_albedo of n world-space points on one Checker or Noise sphere of the scene (see rtk::rt_solid_probe)
extern "C" int rt_hip_solid_probe(RtHipScene* s, uint32_t sphere, const double* d_points, float* d_rgb, uint32_t n, void* stream) {
  if (!s || !d_points || !d_rgb) return fail(RT_ERR_INVALID, "null argument");
  const std::vector<RtSphere>& sp = s->res->sph.spheres;
  if (sphere >= sp.size() || sphere >= s->dev.n_spheres) return fail(RT_ERR_INVALID, "the sphere index lies outside the scene");
  if (sp[sphere].kind != RT_MAT_CHECKER && sp[sphere].kind != RT_MAT_NOISE) return fail(RT_ERR_INVALID, "the sphere is neither Checker nor Noise");
  if (!n) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_solid_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->dev, sphere, d_points, d_rgb, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// hit_world with the medium candidate of n rays on the device, one per thread, through the scene's tables (see rtk::rt_medium_probe)
extern "C" int rt_hip_medium_probe(RtHipScene* s, const double* d_rays, const float* d_tau, const uint32_t* d_node, double* d_t, int32_t* d_best,
                                   uint32_t* d_work, uint32_t n, void* stream) {
  if (!s || !d_rays || !d_node || !d_t || !d_best) return fail(RT_ERR_INVALID, "null argument");
  if (!s->dev.medium) return fail(RT_ERR_INVALID, "the scene has no media");
  if (!n) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_medium_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->dev, d_rays, d_tau, d_node, d_t, d_best, d_work, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// The device form of the aim at an emitting flat primitive (include/rt_abi_test_flat_light.h), one activation per thread.
namespace rtk {
// activation i = {pixel, sample, node of the hit} shooting light j[i] of the scene: what lane_aim_light's flat arm does — the light list, the
// entry's resident record and limit, child_node, the cold flat_light_point — and T comes back; a j that is not an emitter gives three NaNs
__global__ void rt_flat_light_probe(const rtc::DevScene sc, const uint32_t* act, const uint32_t* j, double* T, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rtc::V3 t = rtc::v3(rtc::rt_nan(), rtc::rt_nan(), rtc::rt_nan());
  const uint32_t lj = j[i];
  if (lj < sc.n_lights && sc.lights[lj] >= sc.n_spheres) {
    const uint32_t k = sc.lights[lj] - sc.n_spheres;
    const rtc::RngAddr ra{act[3u * i], act[3u * i + 1u], sc.seed_lo, sc.seed_hi};
    t = rtc::flat_light_point(sc.quads.rec + k, sc.quads.lim ? sc.quads.lim + k : nullptr, ra, rtc::child_node(act[3u * i + 2u], lj));
  }
  T[3u * i] = t.x; T[3u * i + 1u] = t.y; T[3u * i + 2u] = t.z;
}
// rt_flat_light_aim of activation i on ITS OWN entry quv[i] (q, u, v), shape and four words: the header's arithmetic on crafted tables
__global__ void rt_flat_light_aim_probe(const double* quv, const int32_t* triangle, const uint32_t* words, double* T, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rt_flat_light_aim(quv + 9u * (size_t)i, quv + 9u * (size_t)i + 3, quv + 9u * (size_t)i + 6, triangle[i] != 0, words + 4u * (size_t)i, T + 3u * (size_t)i);
}
}  // namespace rtk
extern "C" int rt_hip_flat_light_probe(RtHipScene* s, const double* d_P, const uint32_t* d_pixel_sample_node, const uint32_t* d_j, double* d_T, uint32_t n,
                                       void* stream) {
  (void)d_P;   // (the aim point does not depend on where the light ray starts: d = T - P is the caller's subtraction)
  if (!s || !d_pixel_sample_node || !d_j || !d_T) return fail(RT_ERR_INVALID, "null argument");
  if (s->res->flat_lights.empty()) return fail(RT_ERR_INVALID, "the scene has no emitting flat primitive");
  if (!n) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_flat_light_probe, dim3((n + 191) / 192), dim3(192), 0, (hipStream_t)stream, s->dev, d_pixel_sample_node, d_j, d_T, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
// (block: the launch's workgroup size, 1 .. 1024; a test passes one that is not a multiple of 64)
extern "C" int rt_hip_flat_light_aim_probe(const double* d_quv, const int32_t* d_triangle, const uint32_t* d_words, double* d_T, uint32_t n, uint32_t block,
                                           void* stream) {
  if (!d_quv || !d_triangle || !d_words || !d_T) return fail(RT_ERR_INVALID, "null argument");
  if (block < 1u || block > 1024u) return fail(RT_ERR_INVALID, "block must be 1 .. 1024");
  if (!n) return RT_OK;
  hipLaunchKernelGGL(rtk::rt_flat_light_aim_probe, dim3((n + block - 1u) / block), dim3(block), 0, (hipStream_t)stream, d_quv, d_triangle, d_words, d_T, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// The device form of the image lookup (include/rt_abi_test_flat_image.h), one hit per thread.
namespace rtk {
// hit i at P[i] on entry k[i] whose origin is origin[i]: what the arm in lane_shade does — the header in front of the records, the cold
// flat_image_albedo — and the attenuation comes back; a k outside the entries gives three NaNs
__global__ void rt_flat_image_probe(const rtc::DevScene sc, const uint32_t* k, const double* origin, const double* P, float* out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rtc::Rgb c = rtc::rgb((float)rtc::rt_nan(), (float)rtc::rt_nan(), (float)rtc::rt_nan());
  if ((sc.n_tris & rtc::FLAT_IMAGES_BIT) && k[i] < sc.n_quads)
    c = rtc::flat_image_albedo(reinterpret_cast<const rtc::FlatBvhHeader*>(sc.quads.rec) - 1, k[i], rtc::v3(origin[3u * i], origin[3u * i + 1u], origin[3u * i + 2u]),
                               rtc::v3(P[3u * i], P[3u * i + 1u], P[3u * i + 2u]));
  out[3u * i] = c.r; out[3u * i + 1u] = c.g; out[3u * i + 2u] = c.b;
}
// rt_flat_image_texel of hit i on ITS OWN record, frame and point: the header's arithmetic on crafted tables
__global__ void rt_flat_image_texel_probe(const RtFlatImageRec* rec, const double* ouvw, const double* P, uint32_t* texel, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const RtFlatImageRec r = rec[i];
  if (r.W == 0u || r.H == 0u) { texel[3u * i] = texel[3u * i + 1u] = texel[3u * i + 2u] = 0xFFFFFFFFu; return; }
  const double* f = ouvw + 12u * (size_t)i;
  const RtFlatImageTexel x = rt_flat_image_texel(r, f, f + 3, f + 6, f + 9, P + 3u * (size_t)i);
  texel[3u * i] = x.col; texel[3u * i + 1u] = x.row; texel[3u * i + 2u] = x.index;
}
}  // namespace rtk
extern "C" int rt_hip_flat_image_probe(RtHipScene* s, const uint32_t* d_k, const double* d_origin, const double* d_P, float* d_rgb, uint32_t n, void* stream) {
  if (!s || !d_k || !d_origin || !d_P || !d_rgb) return fail(RT_ERR_INVALID, "null argument");
  if (!s->res->flat.n_images) return fail(RT_ERR_INVALID, "the scene has no flat primitive with an image");
  if (!n) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_flat_image_probe, dim3((n + 191) / 192), dim3(192), 0, (hipStream_t)stream, s->dev, d_k, d_origin, d_P, d_rgb, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
// (block: the launch's workgroup size, 1 .. 1024; a test passes one that is not a multiple of 64)
extern "C" int rt_hip_flat_image_texel_probe(const void* d_rec, const double* d_ouvw, const double* d_P, uint32_t* d_texel, uint32_t n, uint32_t block, void* stream) {
  if (!d_rec || !d_ouvw || !d_P || !d_texel) return fail(RT_ERR_INVALID, "null argument");
  if (block < 1u || block > 1024u) return fail(RT_ERR_INVALID, "block must be 1 .. 1024");
  if (!n) return RT_OK;
  hipLaunchKernelGGL(rtk::rt_flat_image_texel_probe, dim3((n + block - 1u) / block), dim3(block), 0, (hipStream_t)stream,
                     static_cast<const RtFlatImageRec*>(d_rec), d_ouvw, d_P, d_texel, n);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}

// The device surface of flat primitives that move within the frame (include/rt_abi_test_flat_motion.h), one ray per thread.
namespace rtk {
// ray i at shutter time tau[i] (null: 0) with its own closest-so-far and the hit it already holds (null: -1): what a QUADS ∧ MOTION
// megakernel does for a segment — the motion tables at tau, flats_hit through them (flats_hit_shutter: the scan, the structure or the moving
// walk behind the scene's bits), then object_surface<true> of a newly accepted flat entry (the cold flat_surface_shutter where the scene has
// shading normals or motion records) — without the megakernel around it.  out_best is always written; t, P, the normal, front_face and the
// origin left in g.cx, g.cy, g.cz only for an accepted flat entry that is not the hit the ray came with.
__global__ void rt_flat_shutter_probe(const rtc::DevScene sc, const double* rays, const float* tau, const double* closest, const int32_t* best_in, uint32_t n,
                                      int32_t* out_best, double* out_t, double* out_point, double* out_normal, int32_t* out_front, double* out_origin) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const rtc::V3 o = rtc::v3(rays[6u * (size_t)i], rays[6u * (size_t)i + 1u], rays[6u * (size_t)i + 2u]);
  const rtc::V3 d = rtc::v3(rays[6u * (size_t)i + 3u], rays[6u * (size_t)i + 4u], rays[6u * (size_t)i + 5u]);
  const rtc::GlobalTables still{sc.geom, sc.matc};
  const auto tb = rtc::motion_tables(still, sc.motion, tau ? tau[i] : 0.0f);
  const int held = best_in ? best_in[i] : -1;
  const rtc::HitCB r = rtc::flats_hit(sc, tb, o, d, closest[i], held);
  out_best[i] = r.best;
  // (an id the walk accepted lies in n_spheres .. n_spheres + n_quads - 1; the one that came in may be anything and is never looked up)
  if (r.best == held || r.best < 0 || (uint32_t)r.best < sc.n_spheres || (uint32_t)r.best - sc.n_spheres >= sc.n_quads) return;
  rtc::SphereGeom g;
  const rtc::Surface s = rtc::object_surface<true>(sc, tb, o, d, r.closest, (uint32_t)r.best, 0.0, g);
  out_t[i] = r.closest;
  out_point[3u * (size_t)i] = s.point.x; out_point[3u * (size_t)i + 1u] = s.point.y; out_point[3u * (size_t)i + 2u] = s.point.z;
  out_normal[3u * (size_t)i] = s.normal.x; out_normal[3u * (size_t)i + 1u] = s.normal.y; out_normal[3u * (size_t)i + 2u] = s.normal.z;
  out_front[i] = s.front_face ? 1 : 0;
  out_origin[3u * (size_t)i] = g.cx; out_origin[3u * (size_t)i + 1u] = g.cy; out_origin[3u * (size_t)i + 2u] = g.cz;
}
}  // namespace rtk
// (block: the launch's workgroup size, 1 .. 1024.  A scene without motion tables would not select a MOTION kernel, and one without flat
//  primitives has no records to put a header in front of: both are refused before anything is launched)
extern "C" int rt_hip_flat_shutter_probe(RtHipScene* s, const double* d_rays, const float* d_tau, const double* d_closest, const int32_t* d_best_in,
                                         uint32_t n, uint32_t block, int32_t* d_best, double* d_t, double* d_point, double* d_normal, int32_t* d_front,
                                         double* d_origin, void* stream) {
  if (!s || !d_rays || !d_closest || !d_best || !d_t || !d_point || !d_normal || !d_front || !d_origin) return fail(RT_ERR_INVALID, "null argument");
  if (block < 1u || block > 1024u) return fail(RT_ERR_INVALID, "block must be 1 .. 1024");
  if (!s->res->flat.n_quads || !s->dev.n_quads || !s->dev.quads.rec) return fail(RT_ERR_INVALID, "the scene has no flat primitive");
  if (!s->dev.motion) return fail(RT_ERR_INVALID, "nothing in the scene moves within the frame: it selects no MOTION kernel");
  if (!n) return RT_OK;
  RT_HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(rtk::rt_flat_shutter_probe, dim3((uint32_t)(((uint64_t)n + block - 1u) / block)), dim3(block), 0, (hipStream_t)stream, s->dev, d_rays, d_tau, d_closest,
                     d_best_in, n, d_best, d_t, d_point, d_normal, d_front, d_origin);
  RT_HIP_TRY(hipGetLastError());
  return RT_OK;
}
#endif  // RT_TEST_PROBES
