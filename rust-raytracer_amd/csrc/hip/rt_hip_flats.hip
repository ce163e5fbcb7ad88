// rt_hip_flats.hip — changing the flat primitives of a resident scene: the geometry (rt_hip_scene_update_flats), the
// shading normals (§25), the motion within the frame (§27), the emission (§28) and the images (§29).  Part of rt_hip_api.hip's translation
// unit (included there, as rt_hip_group.hip is).  The five entry points share ONE path (§24 "One update path"): flat_call_begin checks the
// arguments and drains the scene, a Flats::HeaderState describes the generation being built, and flats_go_live places the records, writes
// the header — once, with its final values — and swaps the generation in.  Everything that can fail runs before anything the scene renders
// with changes.
namespace {
using Flats = RtHipScene::Resident::Flats;

// ------------------------------------------------------------------------------ the preamble
// An entry point as its refusals name it: the group's call of the same name, the verb of the shared-view message, the flags it knows, the
// alignment of its table in device memory and that argument's name.
struct FlatCall {
  const char *name, *group_name, *through;
  uint32_t flags;
  uintptr_t align;
  const char* arg;
};
constexpr FlatCall UPDATE_FLATS = {"rt_hip_scene_update_flats", "rt_hip_group_update_flats", "updates through", RT_UPDATE_FLATS_REBUILD | RT_UPDATE_FLATS_DEVICE, 8, "quv"};
constexpr FlatCall SET_FLAT_MOTION = {"rt_hip_scene_set_flat_motion", "rt_hip_group_set_flat_motion", "updates through", RT_UPDATE_FLATS_DEVICE, 8, "move"};
constexpr FlatCall SET_FLAT_NORMALS = {"rt_hip_scene_set_flat_normals", "rt_hip_group_set_flat_normals", "sets them through", RT_UPDATE_FLATS_DEVICE, 8, "normals"};
constexpr FlatCall SET_FLAT_LIGHTS = {"rt_hip_scene_set_flat_lights", "rt_hip_group_set_flat_lights", "sets them through", RT_UPDATE_FLATS_DEVICE, 4, "emit"};
constexpr FlatCall SET_FLAT_IMAGES = {"rt_hip_scene_set_flat_images", "rt_hip_group_set_flat_images", "sets them through", RT_UPDATE_FLATS_DEVICE, 8, "images"};

// The checks every entry point starts with, in the order that decides which message a doubly wrong call gets; then *on_device (the table
// is device memory) and the scene drained on its device.  views_follow: the caller (the group) re-points the views that share this scene's
// tables itself.
int flat_call_begin(RtHipScene* s, const FlatCall& c, const void* table, uint32_t n_quads, uint32_t flags, bool views_follow, bool* on_device) {
  if (!s) return fail(RT_ERR_INVALID, "null argument");
  const std::string who = c.name;
  if (flags & ~c.flags) return fail(RT_ERR_INVALID, who + ": unknown flag");
  const Flats& f = s->res->flat;
  if (!f.n_quads) return fail(RT_ERR_INVALID, who + ": the scene has no flat primitive");
  if (n_quads != f.n_quads)
    return fail(RT_ERR_INVALID, who + ": n_quads is " + std::to_string(n_quads) + ", the scene has " + std::to_string(f.n_quads) + " flat primitives");
  if (const int refused = check_not_shared(s, views_follow, c.name, c.through, c.group_name)) return refused;
  *on_device = table && (flags & RT_UPDATE_FLATS_DEVICE) != 0u;
  if (*on_device)
    if (const int refused = check_aligned(table, c.align, (who + ": " + c.arg + " must be " + std::to_string(c.align) + "-byte aligned").c_str())) return refused;
  return make_current_and_drain(s);
}

// the caller's table where the kernels read it: device memory as it is, host memory uploaded into `staging`, null as that many zero bytes
int flat_input(const void* table, size_t bytes, bool on_device, DevBuf& staging, const void** dev) {
  *dev = table;
  if (on_device) return RT_OK;
  if (const int rc = room(staging, bytes)) return rc;
  if (table) RT_HIP_TRY(hipMemcpy(staging.p, table, bytes, hipMemcpyHostToDevice));
  else RT_HIP_TRY(hipMemset(staging.p, 0, bytes));
  *dev = staging.p;
  return RT_OK;
}

// ------------------------------------------------------------------------------ the transition
// From the live generation to `next`: the records where next's header count puts them, the header in front of them, the swap.  placed: the
// first of the records the caller built, in the spare behind next.slot() slots; null: the records stay as they are — in place, or, where a
// scan scene gains or loses the header's slot, copied device to device into the spare.  The ONE fallback: an update has to place its records
// before the readback says whether any entry moves (next.n_moving), so a scan scene whose motion table comes out empty and has no other
// table finds them one slot too far back; they are copied once more, through Scratch::rec_tmp.  The header is written here and nowhere
// else, from Flats::keep_header, which lives as long as the scene.  A table of `next` that is not the live buffer is swapped in.
int flats_go_live(RtHipScene* s, const Flats::HeaderState& next, const RtQuadRec* placed) {
  Flats& f = s->res->flat;
  Flats::Tables& spare = f.spare;
  const size_t n = f.n_quads, has = next.slot();
  DevBuf* into = placed ? &spare.rec : &f.live.rec;   // the buffer that holds the next generation's records
  const RtQuadRec* from = placed ? placed : f.first_rec(f.live);
  if (from != into->get<RtQuadRec>() + has) {
    DevBuf& other = placed ? f.scratch.rec_tmp : spare.rec;
    if (const int rc = room(other, (n + has) * sizeof(RtQuadRec))) return rc;
    RT_HIP_TRY(hipMemcpy(other.get<RtQuadRec>() + has, from, n * sizeof(RtQuadRec), hipMemcpyDeviceToDevice));
    if (placed) spare.rec.swap(other);
    into = &spare.rec;
  }
  if (has) {
    f.keep_header = f.header(next, into->get<RtQuadRec>() + has, s->host.n_spheres);
    RT_HIP_TRY(hipMemcpy(into->p, &f.keep_header, sizeof f.keep_header, hipMemcpyHostToDevice));
  }
  RT_HIP_TRY(hipDeviceSynchronize());
  // everything is built: swap it in (nothing above changed what the scene renders with)
  if (into == &spare.rec) f.live.rec.swap(spare.rec);
  if (next.nodes != &f.live.nodes) f.live.nodes.swap(spare.nodes);
  if (next.order != &f.live.order) f.live.order.swap(spare.order);
  if (next.normals != &f.normals) f.normals.swap(f.normals_spare);
  if (next.motion != &f.motion) f.motion.swap(f.motion_spare);
  if (next.images != &f.images) f.images.swap(f.images_spare);
  f.n_nodes = next.n_nodes; f.n_normals = next.n_normals; f.n_moving = next.n_moving; f.n_images = next.n_images;
  return RT_OK;
}

// ------------------------------------------------------------------------------ moving the flat primitives
// What an update makes the next records from, in device memory: the q, u, v of every entry and the doubles from one entry's to the next's;
// the displacements likewise — null: the scene has no motion table and gets none, else one is produced (and the finite check's message
// speaks of displacements); whether the caller asked for the structure to be built anew.
struct FlatUpdate {
  const double* quv = nullptr;
  uint32_t quv_stride = 9;
  const double* move = nullptr;
  uint32_t move_stride = 3;
  bool rebuild = false;
};
// The update itself, behind rt_hip_scene_update_flats and rt_hip_scene_set_flat_motion.  host_records(rec, device records): the records of
// the new geometry on the host, for a host rebuild — derived from the caller's geometry, or the device's read back.
template <typename HostRecords>
int flats_update(RtHipScene* s, const FlatUpdate& in, rtp::Clock& pc, HostRecords&& host_records) {
  Flats& f = s->res->flat;
  Flats::Tables& spare = f.spare;
  Flats::Scratch& fb = f.scratch;
  const uint32_t n = f.n_quads;
  const bool bvh = f.n_nodes != 0u, with_move = in.move != nullptr;
  bool rebuild = bvh && in.rebuild;
  const bool device_build = rebuild && s->opt.flat_build == 1;   // (§26: the order table on the device; a changed refused set still goes to the host)
  // the generation this update builds: its own nodes and motion table beside the tables that stay.  (§27) how many entries move is known
  // after the readback: the records are placed for a motion table that has some (flats_go_live's fallback covers the one that has none)
  Flats::HeaderState next = f.state();
  if (bvh) next.nodes = &spare.nodes;
  if (with_move) next.motion = &f.motion_spare;
  next.n_moving = with_move ? 1u : 0u;
  const uint32_t slot = next.slot();
  int rc;
  if ((rc = room(spare.rec, ((size_t)n + slot) * sizeof(RtQuadRec))) != RT_OK || (rc = room(fb.status, sizeof(rtfb::Status))) != RT_OK ||
      (with_move && (rc = room(f.motion_spare, (size_t)n * 32)) != RT_OK) ||
      (bvh && ((rc = room(fb.box, (size_t)n * 48)) != RT_OK || (rc = room(spare.nodes, (size_t)f.n_nodes * sizeof(rtc::FlatNode))) != RT_OK)))
    return rc;
  if (with_move) {  // the MOTION kernels' dv table while no sphere moves, now or after a later rt_hip_scene_update_spheres: every word -0.0
    const size_t words = 4 * (size_t)(s->host.n_spheres ? s->host.n_spheres : 1u);
    if (f.still.cap < words * 8) {
      if ((rc = room(f.still, words * 8)) != RT_OK) return rc;
      const std::vector<double> still(words, -0.0);
      RT_HIP_TRY(hipMemcpy(f.still.p, still.data(), words * 8, hipMemcpyHostToDevice));
    }
  }
  rtfb::BuildJob bj;
  if (device_build) {  // the boxed entries in index order, uploaded once per host build; scratch and the spare order table, allocated once
    if (!f.start_ready) {
      f.keep_start.clear();
      for (uint32_t k = 0; k < n; ++k) if (f.topo.boxed[k]) f.keep_start.push_back(k);
      if ((rc = upload(f.start, f.keep_start)) != RT_OK) return rc;
      f.start_ready = true;
    }
    bj.n = n; bj.m = (uint32_t)f.keep_start.size();
    RT_HIP_TRY(rtfb::build_sort_bytes(bj.m, &bj.sort_bytes));
    if ((rc = room(spare.order, (size_t)n * sizeof(uint32_t))) != RT_OK || (rc = room(fb.item, (size_t)bj.m * sizeof(rtc::FlatBuildItem))) != RT_OK ||
        (rc = room(fb.extent, rtfb::build_extent_bytes(bj.m))) != RT_OK || (rc = room(fb.sort_tmp, bj.sort_bytes)) != RT_OK)
      return rc;
  }
  pc.mark("update_flats.upload");
  rtfb::Job j;
  j.n = n;
  j.quv = in.quv; j.quv_stride = in.quv_stride;
  if (with_move) { j.move = in.move; j.move_stride = in.move_stride; j.motion = f.motion_spare.get<double>(); }
  j.lim = f.dev_lim();
  j.rec = spare.rec.get<RtQuadRec>() + slot;
  j.status = fb.status.get<rtfb::Status>();
  if (bvh) {
    const rtc::FlatTopology& tp = f.topo;
    j.boxed = f.boxed.get<const uint32_t>(); j.box = fb.box.get<double>();
    j.n_nodes = f.n_nodes; j.n_run = tp.n_run; j.n_leaves = (uint32_t)tp.leaves.size();
    j.live_nodes = f.live.nodes.get<const rtc::FlatNode>(); j.order = f.live.order.get<const uint32_t>();
    j.leaves = f.leaves.get<const uint32_t>(); j.level_nodes = f.levels.get<const uint32_t>();
    j.level_start = tp.level_start.data(); j.n_levels = (uint32_t)tp.level_start.size() - 1u;
    j.nodes = spare.nodes.get<rtc::FlatNode>();
  }
  RT_HIP_TRY(rtfb::prepare(j, nullptr));
  if (device_build) {  // (enqueued before the readback too: the order table into the spare, then the refit over it — the skeleton is the live one)
    bj.box = fb.box.get<const double>(); bj.start = f.start.get<const uint32_t>(); bj.live_order = f.live.order.get<const uint32_t>();
    bj.item = fb.item.get<rtc::FlatBuildItem>(); bj.extent = fb.extent.get<unsigned long long>(); bj.sort_tmp = fb.sort_tmp.p;
    bj.order = spare.order.get<uint32_t>();
    RT_HIP_TRY(rtfb::build(bj, nullptr));
    j.order = bj.order;
    RT_HIP_TRY(rtfb::refit(j, nullptr));
  } else if (bvh && !rebuild) {  // (enqueued before the readback: a refit the status then rejects was written into spares and is dropped)
    RT_HIP_TRY(rtfb::refit(j, nullptr));
  }
  rtfb::Status st;
  RT_HIP_TRY(hipMemcpy(&st, fb.status.p, sizeof st, hipMemcpyDeviceToHost));  // the one readback: the first bad entry of each class, changed flags
  pc.mark("update_flats.kernels_and_readback");
  if (st.bad_finite != rtfb::NONE || st.bad_degenerate != rtfb::NONE) {  // (creation's loop stops at the first bad entry: the lowest index wins)
    if (st.bad_finite < st.bad_degenerate)
      return fail(RT_ERR_INVALID, "quad " + std::to_string(st.bad_finite) + (with_move ? ": q, u, v, the displacement and q + displacement must be finite" : ": q, u and v must be finite"));
    return fail(RT_ERR_INVALID, "quad " + std::to_string(st.bad_degenerate) + ": degenerate (|cross(u, v)|^2 is zero, subnormal or not finite)");
  }
  next.n_moving = with_move ? st.pad : 0u;
  if (bvh && st.mismatch) rebuild = true;  // an entry became a needle, crossed 2^40 (§27: at either end of its motion), or stopped being one: the order table is another
  const bool built = device_build && !st.mismatch;  // the device's order table stands; with a mismatch the counts are others: the host builds
  if (rebuild) next.order = &spare.order;
  if (rebuild && !built) {  // the host's build_flat_bvh over the host's records, as creation runs it; the records themselves stay the device's
    rtc::HostTables t;
    t.quads.resize(n);
    if ((rc = host_records(t.quads, j.rec)) != RT_OK) return rc;
    if (next.n_moving) {  // (§27: the builder sweeps the boxes with the records the device just made)
      t.flat_motion.resize(4 * (size_t)n);
      RT_HIP_TRY(hipMemcpy(t.flat_motion.data(), f.motion_spare.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    }
    t.quad_lim = f.host_lim;
    const std::string why = rtc::build_flat_bvh(t);
    if (!why.empty()) return fail(RT_ERR_INVALID, why);
    f.keep_nodes.assign(t.flat_nodes.begin(), t.flat_nodes.end());
    f.keep_order.assign(t.flat_order.begin(), t.flat_order.end());
    next.n_nodes = (uint32_t)f.keep_nodes.size();
    pc.mark("update_flats.host_build");
    if ((rc = upload_flat_structure(f, spare, f.keep_nodes, f.keep_order, t.flat_always)) != RT_OK) return rc;
    pc.mark("update_flats.upload_structure");
  }
  if ((rc = flats_go_live(s, next, j.rec)) != RT_OK) return rc;
  f.refits = (bvh && !rebuild) ? f.refits + 1u : 0u;
  if (built) f.device_builds++;
  rc = adopt_tables(s, Moved::flats);
  pc.mark("update_flats.configuration");
  return rc;
}

// the geometry update: quv, [n_quads][9] in host or (RT_UPDATE_FLATS_DEVICE) device memory, is uploaded once; the motion stays as set — its
// records are made anew beside the new geometry's (Dm follows the new normal)
int scene_update_flats(RtHipScene* s, const double* quv, uint32_t n_quads, uint32_t flags, bool views_follow) {
  if (!quv) return fail(RT_ERR_INVALID, "null argument");
  bool on_device;
  if (const int refused = flat_call_begin(s, UPDATE_FLATS, quv, n_quads, flags, views_follow, &on_device)) return refused;
  rtp::Clock pc = rtp::begin();
  Flats& f = s->res->flat;
  const uint32_t n = n_quads;
  const void* dev_quv;
  if (const int rc = flat_input(quv, (size_t)n * 72, on_device, f.scratch.quv, &dev_quv)) return rc;  // (the geometry travels once)
  FlatUpdate in;
  in.quv = static_cast<const double*>(dev_quv);
  if (f.n_moving) { in.move = f.motion.get<const double>(); in.move_stride = 4u; }
  in.rebuild = (flags & RT_UPDATE_FLATS_REBUILD) != 0u;
  return flats_update(s, in, pc, [&](std::vector<RtQuadRec>& rec, const RtQuadRec*) -> int {
    const double* host_quv = quv;
    if (on_device) {
      f.keep_quv.resize(9 * (size_t)n);
      RT_HIP_TRY(hipMemcpy(f.keep_quv.data(), quv, (size_t)n * 72, hipMemcpyDeviceToHost));
      host_quv = f.keep_quv.data();
    }
    for (uint32_t k = 0; k < n; ++k)
      if (rt_quad_prepare(host_quv + 9 * (size_t)k, host_quv + 9 * (size_t)k + 3, host_quv + 9 * (size_t)k + 6, &rec[k]))
        return fail(RT_ERR_INVALID, "quad " + std::to_string(k) + ": the host refuses an entry the device accepted");
    return RT_OK;
  });
}

// flat primitives that move within the frame: the same update with the geometry the scene has — the live records are the
// input — and `move`, [n_quads][3] in host or (RT_UPDATE_FLATS_DEVICE) device memory, null: all zeros, as the displacements
int scene_set_flat_motion(RtHipScene* s, const double* move, uint32_t n_quads, uint32_t flags, bool views_follow) {
  bool on_device;
  if (const int refused = flat_call_begin(s, SET_FLAT_MOTION, move, n_quads, flags, views_follow, &on_device)) return refused;
  Flats& f = s->res->flat;
  const uint32_t n = n_quads;
  if (move && !s->res->flat_lights.empty()) {  // (§28: an emitter cannot move, as a Light sphere cannot; only a scene that has one looks)
    std::vector<double> dev_move;
    if (on_device) {
      dev_move.resize(3 * (size_t)n);
      RT_HIP_TRY(hipMemcpy(dev_move.data(), move, (size_t)n * 24, hipMemcpyDeviceToHost));
    }
    const double* m = on_device ? dev_move.data() : move;
    for (uint32_t k : s->res->flat_lights)   // (entry order: the lowest first)
      if (!(m[3 * (size_t)k] == 0.0 && m[3 * (size_t)k + 1] == 0.0 && m[3 * (size_t)k + 2] == 0.0))
        return fail(RT_ERR_INVALID, "quad " + std::to_string(k) + ": an emitting flat primitive cannot move");
  }
  if (!move && !f.n_moving) return RT_OK;   // nothing moves and nothing shall: the scene is what it was
  rtp::Clock pc = rtp::begin();
  const void* dev_move;
  if (const int rc = flat_input(move, (size_t)n * 24, on_device, f.scratch.move, &dev_move)) return rc;
  FlatUpdate in;
  in.quv = reinterpret_cast<const double*>(f.first_rec(f.live)); in.quv_stride = 16u;  // (a record begins with its q, u, v)
  in.move = static_cast<const double*>(dev_move);
  return flats_update(s, in, pc, [&](std::vector<RtQuadRec>& rec, const RtQuadRec* dev_rec) -> int {  // (the records as they are)
    RT_HIP_TRY(hipMemcpy(rec.data(), dev_rec, (size_t)n * sizeof(RtQuadRec), hipMemcpyDeviceToHost));
    return RT_OK;
  });
}

// ------------------------------------------------------------------------------ shading normals on the triangles
// The records are made on the device from host or device input alike (rt_flat_build.hip: one code path, one table); the table's address
// travels in the header (flats_go_live).
int scene_set_flat_normals(RtHipScene* s, const double* normals, uint32_t n_quads, uint32_t flags, bool views_follow) {
  bool on_device;
  if (const int refused = flat_call_begin(s, SET_FLAT_NORMALS, normals, n_quads, flags, views_follow, &on_device)) return refused;
  Flats& f = s->res->flat;
  Flats::Scratch& fb = f.scratch;
  const uint32_t n = n_quads;
  Flats::HeaderState next = f.state();
  next.n_normals = 0;
  int rc;
  if (normals) {
    const void* in;
    if ((rc = room(f.normals_spare, (size_t)n * 72)) != RT_OK || (rc = room(fb.status, sizeof(rtfb::Status))) != RT_OK ||
        (rc = flat_input(normals, (size_t)n * 72, on_device, fb.quv, &in)) != RT_OK)
      return rc;
    rtfb::NormalJob j;
    j.n = n; j.in = static_cast<const double*>(in); j.lim = f.dev_lim();
    j.out = f.normals_spare.get<double>(); j.status = fb.status.get<rtfb::Status>();
    RT_HIP_TRY(rtfb::normals(j, nullptr));
    rtfb::Status st;
    RT_HIP_TRY(hipMemcpy(&st, fb.status.p, sizeof st, hipMemcpyDeviceToHost));  // the one readback: the lowest bad entry of each class, the count
    if (st.bad_finite != rtfb::NONE || st.bad_degenerate != rtfb::NONE) {
      if (st.bad_finite < st.bad_degenerate)
        return fail(RT_ERR_INVALID, "quad " + std::to_string(st.bad_finite) + ": normal vectors must be finite, with a squared length that is finite, normal and not zero");
      return fail(RT_ERR_INVALID, "quad " + std::to_string(st.bad_degenerate) + ": normal vectors on a parallelogram (only triangles interpolate)");
    }
    next.n_normals = st.mismatch;
    if (next.n_normals) next.normals = &f.normals_spare;
  }
  if ((rc = flats_go_live(s, next, nullptr)) != RT_OK) return rc;
  return adopt_tables(s, Moved::flats);
}

// ------------------------------------------------------------------------------ flat primitives that emit
// The table is small (12 bytes an entry) and checked on the host, from host or device input alike.  What changes on the device: the emitters'
// records of `mat` and `matc` (kind Light, colour `emit`; every other flat record is put back as created) and the light list; no geometry
// table, no header slot — the aim reads the entry's own record.  Everything that can be refused is refused before the scene changes.
int scene_set_flat_lights(RtHipScene* s, const float* emit, uint32_t n_quads, uint32_t flags, bool views_follow) {
  bool on_device;
  if (const int refused = flat_call_begin(s, SET_FLAT_LIGHTS, emit, n_quads, flags, views_follow, &on_device)) return refused;
  RtHipScene::Resident& r = *s->res;
  Flats& f = r.flat;
  int rc;
  const uint32_t n = n_quads, n_spheres = s->host.n_spheres;
  std::vector<float> table(3 * (size_t)n, 0.0f);   // (a null table: all zeros, no entry emits)
  if (on_device) RT_HIP_TRY(hipMemcpy(table.data(), emit, (size_t)n * 12, hipMemcpyDeviceToHost));
  else if (emit) std::memcpy(table.data(), emit, (size_t)n * 12);
  uint32_t n_emit = 0;
  const uint32_t bad = rt_flat_light_emit_check(table.data(), n, &n_emit);
  if (bad != n) return fail(RT_ERR_INVALID, "quad " + std::to_string(bad) + ": every component of emit must be finite and in [0, 1]");
  if (n_emit > RT_MAX_FLAT_LIGHTS) return fail(RT_ERR_UNSUPPORTED, "more than RT_MAX_FLAT_LIGHTS (32) emitting flat primitives: every sampling hit shoots one ray per light");
  if (!n_emit && r.flat_lights.empty()) return RT_OK;   // nothing emits and nothing shall: the scene is what it was
  // the flat primitives' material records and the light list, on the host (rt_tables.h: the CPU builds of the tests make the same tables)
  std::vector<rtc::SphereMat> mat;
  std::vector<rtc::MatCore> matc;
  std::vector<uint32_t> lights, emitters;
  rtc::build_flat_lights(r.keep_flat_mat, r.keep_flat_matc, r.sphere_lights, n_spheres, table.data(), mat, matc, lights, emitters);
  if (n_emit && f.n_moving) {  // an emitter cannot move, as a Light sphere cannot (whichever call comes second refuses)
    std::vector<double> motion(4 * (size_t)n);
    RT_HIP_TRY(hipMemcpy(motion.data(), f.motion.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    for (uint32_t k : emitters)
      if (rt_flat_motion_present(&motion[4 * (size_t)k])) return fail(RT_ERR_INVALID, "quad " + std::to_string(k) + ": an emitting flat primitive cannot move");
  }
  // the pools of the new light count must fit before anything changes (plan_lds reads the count from the scene)
  {
    LdsPlan plan;
    if ((rc = plan_lds(s, s->dev.grid, !lights.empty(), &plan, (int64_t)lights.size())) != RT_OK) return rc;
  }
  DevBuf new_lights;   // (the list may grow: a buffer of its own, swapped in; the old one is freed with this frame, the device idle; the copy
                       //  from pageable memory has returned when upload has)
  if ((rc = upload(new_lights, lights)) != RT_OK) return rc;
  RT_HIP_TRY(hipMemcpy(r.mat.get<rtc::SphereMat>() + n_spheres, mat.data(), mat.size() * sizeof(rtc::SphereMat), hipMemcpyHostToDevice));
  RT_HIP_TRY(hipMemcpy(r.matc.get<rtc::MatCore>() + n_spheres, matc.data(), matc.size() * sizeof(rtc::MatCore), hipMemcpyHostToDevice));
  RT_HIP_TRY(hipDeviceSynchronize());
  r.lights.swap(new_lights);
  r.flat_lights.swap(emitters);
  r.has_lights = r.n_lights() != 0u;
  return adopt_tables(s, Moved::flats);
}

// ------------------------------------------------------------------------------ images on the flat primitives
// As the shading normals: the records are made on the device from host or device input alike (rt_flat_build.hip flat_images_prepare), and the
// table's address — with the texels' — travels in the header (flats_go_live).
int scene_set_flat_images(RtHipScene* s, const RtFlatImage* images, uint32_t n_quads, uint32_t flags, bool views_follow) {
  bool on_device;
  if (const int refused = flat_call_begin(s, SET_FLAT_IMAGES, images, n_quads, flags, views_follow, &on_device)) return refused;
  RtHipScene::Resident& r = *s->res;
  Flats& f = r.flat;
  Flats::Scratch& fb = f.scratch;
  const uint32_t n = n_quads;
  Flats::HeaderState next = f.state();
  next.n_images = 0;
  int rc;
  if (images) {
    static_assert(sizeof(RtFlatImage) == 64 && sizeof(RtFlatImageRec) == 64, "an image entry and its record are 64 bytes");
    const void* in;
    if ((rc = room(f.images_spare, (size_t)n * sizeof(RtFlatImageRec))) != RT_OK || (rc = room(fb.status, sizeof(rtfb::Status))) != RT_OK ||
        (rc = room(fb.kind, (size_t)n * sizeof(uint32_t))) != RT_OK || (rc = flat_input(images, (size_t)n * sizeof(RtFlatImage), on_device, fb.quv, &in)) != RT_OK)
      return rc;
    std::vector<uint32_t> kind(n);   // (the entries' own materials as created: an emitter's resident record says Light meanwhile)
    for (uint32_t k = 0; k < n; ++k) kind[k] = r.keep_flat_matc[k].kind;
    RT_HIP_TRY(hipMemcpy(fb.kind.p, kind.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    rtfb::ImageJob j;
    j.n = n; j.n_textures = f.n_textures; j.in = static_cast<const RtFlatImage*>(in);
    j.tex = f.n_textures ? f.tex_table.get<const RtFlatImageTex>() : nullptr; j.kind = fb.kind.get<const uint32_t>();
    j.out = f.images_spare.get<RtFlatImageRec>(); j.status = fb.status.get<rtfb::Status>();
    RT_HIP_TRY(rtfb::images(j, nullptr));
    rtfb::Status st;
    RT_HIP_TRY(hipMemcpy(&st, fb.status.p, sizeof st, hipMemcpyDeviceToHost));  // the one readback: the lowest refused entry and why, the count
    if (st.bad_degenerate != rtfb::NONE) return fail(RT_ERR_INVALID, "quad " + std::to_string(st.bad_degenerate) + ": " + rt_flat_image_why((int)st.bad_finite));
    next.n_images = st.mismatch;
    if (next.n_images) next.images = &f.images_spare;
  }
  if (!next.n_images && !f.n_images) return RT_OK;   // no entry has an image and none shall: the scene is what it was
  if ((rc = flats_go_live(s, next, nullptr)) != RT_OK) return rc;
  return adopt_tables(s, Moved::flats);
}
}  // namespace

extern "C" int rt_hip_scene_update_flats(RtHipScene* s, const double* quv, uint32_t n_quads, uint32_t flags) {
  return scene_update_flats(s, quv, n_quads, flags, false);
}
extern "C" int rt_hip_scene_set_flat_motion(RtHipScene* s, const double* move, uint32_t n_quads, uint32_t flags) {
  return scene_set_flat_motion(s, move, n_quads, flags, false);
}
extern "C" int rt_hip_scene_set_flat_normals(RtHipScene* s, const double* normals, uint32_t n_quads, uint32_t flags) {
  return scene_set_flat_normals(s, normals, n_quads, flags, false);
}
extern "C" int rt_hip_scene_set_flat_lights(RtHipScene* s, const float* emit, uint32_t n_quads, uint32_t flags) {
  return scene_set_flat_lights(s, emit, n_quads, flags, false);
}
extern "C" int rt_hip_scene_set_flat_images(RtHipScene* s, const RtFlatImage* images, uint32_t n_quads, uint32_t flags) {
  return scene_set_flat_images(s, images, n_quads, flags, false);
}
