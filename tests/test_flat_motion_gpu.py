"""Flat primitives that move while the shutter is open on the GPU, through the C ABI: 48 x 32 frames at spp 4 against the
restatement (tests/flat_motion_mini.py) and against the full scan bit for bit; 1 100 triangles through the swept structure; every
QUADS ∧ MOTION megakernel; the device form of the moving hit test against the host build bit for bit; two checks that need no restatement
(the static bits, the moving black occluder); and the plumbing — set and remove, updates, refit against rebuild, passes, shards, adaptive
frames, the group, every refusal, the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import flat_bvh_sim as F
import flat_motion_frames as MF
import flat_motion_sim
import quad_rays as QR
from parity import assert_parity, pooled_atol
from test_medium_gpu import _cfg, _lam, _load, _obj, _one_shot, _same, _stream
from test_quad_gpu import _floor_objs, _quad

LDS, SIMPLE, HL, WIDE, ACCUM, LENS, MOTION, MEDIUM, SOLID, QUADS = (1 << b for b in range(10))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
W, H, SPP = MF.W, MF.H, MF.SPP
FLAT_TABLES = ("quads", "quad_lim", "flat_bvh", "flat_bvh_order", "flat_normals", "flat_motion", "motion")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _scene(pkg, sc, c1=None, lens=None, quads=None, normals=None, move=None, bvh=False, library=None):
    gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=c1, quads=quads, flat_bvh=bvh)
    if lens:
        gs.set_lens(*lens)
    if normals is not None:
        gs.set_flat_normals(normals)
    if move is not None:
        gs.set_flat_motion(move)
    return gs


def _aovs(gs, n=SPP):
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(n, aov.data_ptr(), None, _stream(torch))
    torch.cuda.synchronize()
    return aov.cpu().numpy()


def _tables(gs):
    return {name: gs.table(name) for name in FLAT_TABLES}


def _frames_equal(a, b, what):
    _same(a, b, what)
    assert a[2]["segments"] == b[2]["segments"] > 0, (what, a[2]["segments"], b[2]["segments"])


def _differs(a, b):
    return not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _quv(quads):
    return np.array([list(q.q) + list(q.u) + list(q.v) for q in quads])


# ------------------------------------------------------------------ frames against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("case,bvh", [(c, b) for c in MF.PARITY_CASES for b in (False, True)])
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case, bvh):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against FlatMotionMini; the scene selects the MOTION
    key with or without a moving sphere, "motion" keeps counting spheres; "variant" 1 gives the same frame bit for bit; the AOVs are the
    restatement's in every bit"""
    sc, c1, lens, quads, normals, move = MF.world(host, case)
    gs = _scene(pkg, sc, c1, lens, quads, normals, None, bvh)
    still = _one_shot(torch, gs)
    key = gs.query("last_kernel")
    assert key & QUADS and bool(key & MOTION) == (c1 is not None) and gs.query("flat_motion") == 0 and gs.table("flat_motion") == b""
    gs.set_flat_motion(move)
    n_moving = int((move != 0).any(axis=1).sum())
    assert gs.query("flat_motion") == n_moving > 0 and len(gs.table("flat_motion")) == 32 * len(quads) and (gs.query("flat_bvh") > 0) == bvh
    assert (gs.query("motion") > 0) == (c1 is not None)
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key | MOTION
    assert _differs((rgb, lin), still), "the motion changed nothing"
    m = MF.mini_frame(oracle, abi, host, case)
    print(f"{case} bvh={bvh}: max |linear diff| {float(np.abs(lin - m['lin']).max()):.3g}, segments gpu {st['segments']} mini {m['segments']} - {m['discarded']}")
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(SPP))
    assert st["segments"] == m["segments"] - m["discarded"]
    gs.set_option("variant", 1)
    b = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key | MOTION
    _frames_equal((rgb, lin, st), b, "variant 1")
    gs.set_option("variant", 0)
    if not bvh and case != "room_box":
        want = MF.mini(oracle, abi, sc, c1, lens, quads, normals, move).aovs(SPP)
        got = _aovs(gs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    gs.close()


@pytest.mark.gpu
def test_1100_triangles_half_of_them_moving(pkg, abi, host, torch_cuda):
    """past the scan's cap: the swept structure against "variant" 1 (every entry in file order) bit for bit, and against the CPU build of
    the lane code (tests/flat_motion_sim.py, itself held to the restatement by tests/test_flat_motion_cpu.py) at the parity bar with the
    exact segment count — the restatement's own frame of 1 100 entries would take minutes"""
    sc, c1, lens = _load(host, _cfg(_floor_objs()), W, H, SPP, MF.DEPTH, seed=7)
    base = sc.quads()
    quv, move = MF.many_triangles()
    flats = F.flats_array(abi, np.concatenate([_quv(base), quv]), [0] * len(base) + [1] * len(quv))
    for k in range(len(base)):
        flats[k] = base[k]
    move = np.concatenate([np.zeros((len(base), 3)), move])
    gs = _scene(pkg, sc, quads=flats, move=move, bvh=True)
    assert gs.query("quads") == 1102 and gs.query("flat_motion") == 550 and gs.query("flat_bvh") > 100
    one = _one_shot(torch, gs)
    assert gs.query("last_kernel") & MOTION
    gs.set_option("variant", 1)
    _frames_equal(_one_shot(torch, gs), one, "variant 1")
    gs.close()
    rc, rgb, lin, segs, info, cnt = flat_motion_sim.load(abi).render(sc.c, flats, move, flat_bvh=True)
    assert rc == 0 and info[1] == 550 and cnt["rays_bvh"] > 0
    assert_parity(one[0], one[1], rgb, lin, "1100 triangles", atol=pooled_atol(SPP))
    assert one[2]["segments"] == segs


@pytest.mark.gpu
def test_all_quads_motion_kernels_run_with_the_table(pkg, abi, host, torch_cuda):
    """the mesh cells of tests/test_feature_matrix.py: with a motion table every cell reports its key with MOTION — the 16 QUADS ∧ MOTION
    megakernels and their 16 accumulating twins — the frame differs from the still one, and the grid walk equals the full scan"""
    import test_feature_matrix as FX
    seen = set()
    for s in FX.MESH:
        key = FX._key(s) | MOTION
        sc, c1, lens, quads = FX._world(host, s)
        move = np.zeros((len(quads), 3))
        move[[k for k, q in enumerate(quads) if q.reserved == abi.RT_QUAD_SHAPE_TRIANGLE]] = [0.3, 0.25, -0.2]
        move[1] = [0.0, 0.0, 0.4]
        gs = _scene(pkg, sc, c1, lens, quads)
        still = _one_shot(torch, gs)
        gs.set_flat_motion(move)
        assert gs.query("flat_motion") == int((move != 0).any(axis=1).sum()) >= FX.N_MESH_TRIS
        one = FX._frame_and_passes(torch, gs, key, FX._id(s))          # (asserts last_kernel == key, then key | ACCUM, frames equal)
        seen |= {key, key | ACCUM}
        assert _differs(one, still), FX._id(s)
        gs.set_option("variant", 1)
        _frames_equal(_one_shot(torch, gs), one, FX._id(s) + ": variant 1")
        gs.close()
    assert len(seen) == 32 and all(k & QUADS and k & MOTION for k in seen) and len({k for k in seen if not k & ACCUM}) == 16


# ------------------------------------------------------------------ the device form, bit for bit
def _device_class_world(abi, cls):
    """one list per class of tests/quad_rays.py (tests/flat_shutter_rays.py full_class_world, which the shutter probe's tests reduce): the
    class's entries a device scene can hold (filled up to 100 with generic ones; triangles and parallelograms in turn, every other entry
    moving by about its own size) and all its rays, each with its own tau and moved along with the entry it is aimed at"""
    import flat_shutter_rays
    return flat_shutter_rays.full_class_world(abi, cls)[:5]


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("bvh", [False, True])
@pytest.mark.parametrize("cls", QR.CLASSES)
def test_device_moving_hit_equals_the_host_build(pkg, abi, torch_cuda, cls, bvh):
    """The nine ray classes of tests/quad_rays.py, >= 10^5 rays each, every ray with its own tau, through rt_hip_medium_probe — hit_world of
    the MOTION tables, then flats_hit at the ray's tau; launches of 1 000 threads: 15 waves and a partial one — against the host build of
    the same code (tests/flat_motion_sim.py): the id and every bit of t, through the scan and through the swept structure.
    This probe has no closest-so-far input (every ray starts at f64::MAX) and returns no surface record; tests/test_flat_shutter_gpu.py
    (rt_hip_flat_shutter_probe) compares those ray by ray: a real closest, a hit already held, and P, the normal, front_face
    and the origin at tau of the device form, bit for bit.  The scene's one medium sphere is 10^30 away; a ray that met it is left out
    and counted."""
    from test_quad_rays_gpu import _dev
    quvs, shapes, move, rays, tau = _device_class_world(abi, cls)
    n = len(quvs)
    flats = F.flats_array(abi, quvs, shapes)
    want_best, want_t, cnt = flat_motion_sim.load(abi).list_hit(flats, move, rays, tau, np.full(len(rays), 1.7976931348623157e308), bvh, id_base=1)
    spheres = (abi.RtSphere * 1)()
    spheres[0].center[:] = [0.0, -1e30, 0.0]
    spheres[0].radius, spheres[0].kind, spheres[0].fuzz_or_ior = 0.5, abi.RT_MAT_MEDIUM, 0.01
    spheres[0].albedo[:] = [0.6, 0.5, 0.7]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=2, max_depth=5, sky_mode=abi.RT_SKY_GRADIENT, spheres=spheres,
                     n_spheres=1, seed=4242)
    sc.cam_origin[:] = [0.0, 0.0, 30.0]; sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]; sc.cam_horizontal[:] = [3.0, 0.0, 0.0]; sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=flats, flat_bvh=bvh)
    try:
        gs.set_flat_motion(move)
        assert gs.query("flat_motion") == int((move != 0).any(axis=1).sum()) >= 50
        d_rays, d_tau, d_node = _dev(rays), _dev(tau), _dev(np.zeros(len(rays), np.uint32))
        d_t = torch.zeros(len(rays), dtype=torch.float64, device="cuda:0")
        d_best = torch.full((len(rays),), -7, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        for off in range(0, len(rays), QR.N_R):
            gs.medium_probe(d_rays.data_ptr() + 48 * off, d_node.data_ptr() + 4 * off, d_t.data_ptr() + 8 * off, d_best.data_ptr() + 4 * off,
                            min(QR.N_R, len(rays) - off), d_tau=d_tau.data_ptr() + 4 * off, stream=stream)
        torch.cuda.synchronize()
        best, t = d_best.cpu().numpy(), d_t.cpu().numpy()
    finally:
        gs.close()
    flat = best != 0                       # (rays that did not meet the sphere)
    hit = (want_best >= 0) & flat
    print(f"{cls} bvh={bvh}: {int(hit.sum())} of {len(rays)} rays hit, {int(((want_best[hit] - 1) % 2 == 0).sum())} of them a moving entry; "
          f"{int((~flat).sum())} met the sphere; host: structure {cnt['rays_bvh']} scan {cnt['rays_scan']}")
    assert len(rays) >= 100_000 and (~flat).sum() <= 0.001 * len(rays)
    if cls in QR.STRADDLING:
        assert hit.sum() > 0.02 * len(rays)
    assert np.array_equal(best[flat], want_best[flat]), int((best[flat] != want_best[flat]).sum())
    assert np.array_equal(t.view(np.uint64)[hit], want_t.view(np.uint64)[hit])


# ------------------------------------------------------------------ two checks that need no restatement
@pytest.mark.gpu
def test_exact_1_the_static_bits(pkg, abi, host, torch_cuda):
    """scene A: still flat primitives and one moving sphere hidden behind the camera (the code as it was: key QUADS | MOTION, no table);
    scene B: A plus a 1 mm moving quad hidden behind the camera, so every still entry goes through the new path.  The same frame bit for
    bit and the same segment count"""
    hidden = _obj((0.0, 1.0, 40.0), 0.05, _lam(0.5, 0.5, 0.5), (0.0, 1.2, 40.0))
    speck = dict(_quad((0.0, 1.0, 50.0), (0.001, 0, 0), (0, 0.001, 0), _lam(0.5, 0.5, 0.5)), move=[0.0, 0.002, 0.0])
    frames = {}
    for name, extra in (("A", [hidden]), ("B", [hidden, speck])):
        sc, c1, lens = _load(host, _cfg(_floor_objs(extra=extra)), W, H, SPP, MF.DEPTH, seed=23)
        move = sc.flat_motion()
        assert c1 is not None and (move is not None) == (name == "B")
        gs = _scene(pkg, sc, c1, lens, sc.quads(), None, move)
        frames[name] = _one_shot(torch, gs)
        assert gs.query("last_kernel") & (QUADS | MOTION) == QUADS | MOTION and gs.query("motion") == 1 and gs.query("flat_motion") == (1 if name == "B" else 0)
        gs.close()
    _frames_equal(frames["A"], frames["B"], "a hidden moving quad")


@pytest.mark.gpu
def test_exact_2_the_moving_black_occluder(pkg, abi, host, torch_cuda):
    """a black Lambertian quad in the plane z = 0 covers everything left of its right edge and slides to the right under the sky.  From the
    camera and the geometry: a pixel column's samples meet the plane at x in [x(col), x(col + 1)); the edge sweeps [e, e + m) over tau in
    [0, 1).  Columns covered at every tau are exactly 0 in linear radiance and RGB8; columns never covered equal the quad-free still frame
    bit for bit; the swept columns and one on each side — at most 6 of 48 — are left out, and one of them is partly covered: its mean lies
    strictly between its neighbours'"""
    edge, slide = 0.33, 0.4
    cam = dict(look_from=(0.0, 0.0, 6.0), look_at=(0.0, 0.0, 0.0))
    black = dict(_quad((edge - 40.0, -20.0, 0.0), (40.0, 0, 0), (0, 40.0, 0), _lam(0.0, 0.0, 0.0)), move=[slide, 0.0, 0.0])
    speck = _obj((0.0, 0.0, 90.0), 0.01, _lam(0.5, 0.5, 0.5))            # (behind the camera: both scenes hold one sphere)
    sc, c1, lens = _load(host, _cfg([speck, black], **cam), W, H, SPP, MF.DEPTH, seed=41)
    sky, _, _ = _load(host, _cfg([speck], **cam), W, H, SPP, MF.DEPTH, seed=41)
    c = sc.c
    o, ll, hor, ver = (np.array(list(v)) for v in (c.cam_origin, c.cam_lower_left, c.cam_horizontal, c.cam_vertical))
    assert ver[0] == 0.0 and ver[2] == 0.0 and hor[2] == 0.0 and o[0] == 0.0      # x on the plane depends on the column alone
    t_plane = (0.0 - o[2]) / (ll[2] - o[2])
    x_at = lambda u: o[0] + t_plane * (ll[0] + u * hor[0] - o[0])                   # camera.rs: u = (column + jitter) / (W - 1), jitter in [0, 1)
    col_lo, col_hi = x_at(np.arange(W) / (W - 1.0)), x_at((np.arange(W) + 1.0) / (W - 1.0))
    swept = np.flatnonzero((col_hi > edge) & (col_lo < edge + slide))
    left_out = np.arange(swept.min() - 1, swept.max() + 2)
    assert 1 <= len(swept) and len(left_out) <= 6 and left_out.min() > 0 and left_out.max() < W - 1
    covered, never = np.arange(0, left_out.min()), np.arange(left_out.max() + 1, W)
    assert (col_hi[covered] < edge).all() and (col_lo[never] > edge + slide).all()
    gs = _scene(pkg, sc, quads=sc.quads(), move=sc.flat_motion())
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") & (QUADS | MOTION) == QUADS | MOTION and gs.query("flat_motion") == 1 and gs.query("motion") == 0
    gs.close()
    g0 = pkg.hip.HipScene(sky.ptr, 0)
    s_rgb, s_lin, _ = _one_shot(torch, g0)
    g0.close()
    assert (lin[:, covered].view(np.uint32) == 0).all() and (rgb[:, covered] == 0).all()
    assert np.array_equal(lin[:, never].view(np.uint32), s_lin[:, never].view(np.uint32)) and np.array_equal(rgb[:, never], s_rgb[:, never])
    assert (s_lin[:, never] > 0).all()
    means = lin.astype(np.float64).mean(axis=(0, 2))
    print(f"left out {left_out.tolist()}, swept {swept.tolist()}, column means {np.round(means[left_out.min() - 1:left_out.max() + 2], 4).tolist()}")
    assert any(means[k - 1] < means[k] < means[k + 1] for k in left_out)


# ------------------------------------------------------------------ tables and state
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_set_and_remove(pkg, abi, host, torch_cuda, bvh):
    """motion set and then removed (None, or all zeros): tables byte for byte and frames bit for bit those of a scene that never had any"""
    sc, c1, lens, quads, normals, move = MF.world(host, "glass_pane")
    never = _scene(pkg, sc, c1, lens, quads, normals, None, bvh)
    gs = _scene(pkg, sc, c1, lens, quads, normals, move, bvh)
    want_t, want_f, want_a, key = _tables(never), _one_shot(torch, never), _aovs(never), never.query("last_kernel")
    with_m = _one_shot(torch, gs)
    assert _differs(with_m, want_f) and gs.table("quads") == want_t["quads"] and gs.table("flat_bvh_order") == want_t["flat_bvh_order"]
    assert gs.table("flat_motion") == np.ascontiguousarray(flat_motion_sim.load(abi).prepare(_quv(quads), move)[1]).tobytes()
    if bvh:                                                         # the structure is the host build's over the swept boxes
        nodes, order, _, _ = flat_motion_sim.load(abi).build(quads, move)
        assert gs.table("flat_bvh") == nodes.tobytes() and gs.table("flat_bvh_order") == order.tobytes()
    gs.set_flat_motion(None)
    assert gs.query("flat_motion") == 0 and _tables(gs) == want_t
    _frames_equal(_one_shot(torch, gs), want_f, "removed")
    assert gs.query("last_kernel") == key and not key & MOTION
    assert np.array_equal(_aovs(gs).view(np.uint32), want_a.view(np.uint32))
    gs.set_flat_motion(move)
    gs.set_flat_motion(np.zeros((len(quads), 3)))             # all zeros: no entry moves, no table
    assert gs.query("flat_motion") == 0 and _tables(gs) == want_t
    gs.set_flat_motion(torch.from_numpy(move).to("cuda:0"))   # ... and back, from device memory
    _frames_equal(_one_shot(torch, gs), with_m, "set again")
    gs.close(); never.close()


def _with_geometry(quads, quv):
    out = (type(quads[0]) * len(quads))(*quads)
    for k in range(len(out)):
        out[k].q[:], out[k].u[:], out[k].v[:] = quv[k, 0:3], quv[k, 3:6], quv[k, 6:9]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["scan", "refit", "rebuild", "device_build"])
def test_update_flats_keeps_the_motion_and_equals_a_fresh_scene(pkg, abi, host, torch_cuda, route):
    """update_flats after set_flat_motion: the motion stays as set, its records follow the new normals, the boxes are swept — records,
    motion table and frame those of a fresh scene with both; a refit, a host rebuild and a device build give the same frame, and a
    rebuild's structure is the host build's over the swept boxes byte for byte, whoever built it"""
    sc, c1, lens, quads, normals, move = MF.world(host, "smooth_mesh")
    c, s = np.cos(0.3), np.sin(0.3)
    Rm = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    quv1 = (_quv(quads).reshape(-1, 3, 3) @ Rm.T)
    quv1[:, 0, 1] += 0.15
    quv1 = quv1.reshape(-1, 9)
    n1 = (normals.reshape(-1, 3, 3) @ Rm.T).reshape(-1, 9)
    bvh = route != "scan"
    gs = _scene(pkg, sc, c1, lens, quads, normals, move, bvh)
    before = _one_shot(torch, gs)
    if route == "device_build":
        gs.set_option("flat_build", 1)
    gs.update_flats(quv1, rebuild=route in ("rebuild", "device_build"))
    gs.set_flat_normals(n1)
    assert gs.query("flat_motion") == int((move != 0).any(axis=1).sum())
    fresh = _scene(pkg, sc, c1, lens, _with_geometry(quads, quv1), n1, move, bvh)
    got, want = _one_shot(torch, gs), _one_shot(torch, fresh)
    a, b = _tables(gs), _tables(fresh)
    for name in ("quads", "quad_lim", "flat_normals", "flat_motion", "motion"):
        assert a[name] == b[name], (route, name)
    if route in ("rebuild", "device_build"):   # (the fresh scene's tree is creation's, refit; a rebuild's is the host build's over the swept boxes)
        nodes, order, _, _ = flat_motion_sim.load(abi).build(_with_geometry(quads, quv1), move)
        assert a["flat_bvh"] == nodes.tobytes() and a["flat_bvh_order"] == order.tobytes(), route
        assert gs.query("flat_device_builds") == (1 if route == "device_build" else 0)
    _frames_equal(got, want, route)
    assert _differs(got, before)
    gs.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_a_motion_that_leaves_the_preconditions_rebuilds_the_structure(pkg, abi, host, torch_cuda, device_input):
    """an entry whose far end lies beyond 2^40 joins the always-visited run: set_flat_motion builds the structure anew, as an update does,
    and the frame is the full scan's"""
    sc, c1, lens, quads, normals, move = MF.world(host, "flat_only")
    far = move.copy(); far[1] = [2.0 ** 41, 0.0, 0.0]
    gs = _scene(pkg, sc, c1, lens, quads, normals, move, True)
    order = gs.table("flat_bvh_order")
    gs.set_flat_motion(torch.from_numpy(far).to("cuda:0") if device_input else far)      # (device memory: only the status crosses back)
    nodes, want_order, n_always, _ = flat_motion_sim.load(abi).build(quads, far)
    assert n_always == 1 and gs.table("flat_bvh_order") == want_order.tobytes() != order and gs.table("flat_bvh") == nodes.tobytes()
    one = _one_shot(torch, gs)
    gs.set_option("variant", 1)
    _frames_equal(_one_shot(torch, gs), one, "variant 1")
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_spheres_that_stop_moving_leave_the_flat_motion(pkg, abi, host, torch_cuda, bvh):
    """a scene with moving spheres and moving flat primitives whose spheres are then updated WITHOUT center1: the flat primitives go on
    moving under the MOTION key — tables and frame those of a fresh scene with still spheres and the same motion — and back"""
    sc, c1, lens, quads, normals, move = MF.world(host, "lens_spheres_medium")
    centres = [list(s.center) for s in sc.c.spheres[:sc.c.n_spheres]]
    gs = _scene(pkg, sc, c1, lens, quads, normals, move, bvh)
    both = _one_shot(torch, gs)
    gs.update_spheres(centres)
    fresh = _scene(pkg, sc, None, lens, quads, normals, move, bvh)
    got, want = _one_shot(torch, gs), _one_shot(torch, fresh)
    assert gs.query("motion") == 0 and gs.query("flat_motion") == fresh.query("flat_motion") > 0
    assert gs.query("last_kernel") == fresh.query("last_kernel") and gs.query("last_kernel") & MOTION
    assert _tables(gs) == _tables(fresh)
    _frames_equal(got, want, "spheres stopped")
    assert _differs(got, both)
    gs.update_spheres(centres, c1)
    _frames_equal(_one_shot(torch, gs), both, "spheres move again")
    gs.close(); fresh.close()


@pytest.mark.gpu
def test_composition_is_the_one_shot_frame(pkg, abi, host, torch_cuda):
    """passes (0, 1), (1, 3), (3, 4), row shards {8, r, 3} and rt_hip_render_adaptive_to_host at threshold 0: each the one-shot frame"""
    sc, c1, lens, quads, normals, move = MF.world(host, "solids")
    gs = _scene(pkg, sc, c1, lens, quads, normals, move)
    one = _one_shot(torch, gs)
    acc = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") & (QUADS | MOTION | ACCUM) == QUADS | MOTION | ACCUM
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    frame_rgb, frame_lin, segs = np.zeros_like(one[0]), np.zeros_like(one[1]), 0
    for r in range(3):
        t = abi.RtRowTiles(8, r, 3)
        rows = abi.tiles_global_rows(H, t)
        s_rgb, s_lin, st = _one_shot(torch, gs, t, len(rows))
        frame_rgb[rows], frame_lin[rows] = s_rgb, s_lin
        segs += st["segments"]
    _same(one, (frame_rgb, frame_lin), "row shards")
    assert segs == one[2]["segments"]
    ad_rgb, ad_spp, _ = gs.render_adaptive(0.0, 2)
    assert (ad_spp == SPP).all() and np.array_equal(ad_rgb, one[0])
    gs.close()


@pytest.mark.gpu
def test_group_of_two_equals_one_rank(pkg, abi, host, torch_cuda, monkeypatch):
    sc, c1, lens, quads, normals, move = MF.world(host, "mirror")
    one = _scene(pkg, sc, c1, lens, quads, normals, move)
    want = _one_shot(torch, one)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(sc.ptr, 2, quads=quads)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    try:
        assert grp.size == 2
        still, _ = grp.render_to_host()
        assert not np.array_equal(still, want[0])
        bad = move.copy(); bad[1, 2] = np.inf
        with pytest.raises(pkg.host.RtError) as e:
            grp.set_flat_motion(bad)
        assert "quad 1:" in str(e.value) and np.array_equal(grp.render_to_host()[0], still)
        grp.set_flat_motion(move)
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])       # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want[0]) and st["segments"] == want[2]["segments"]
        grp.set_flat_motion(None, len(quads))
        assert np.array_equal(grp.render_to_host()[0], still)
    finally:
        grp.close(); one.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(pkg, abi, host, torch_cuda):
    sc, c1, lens, quads, normals, move = MF.world(host, "smooth_mesh")
    L = pkg.hip.lib()
    for bvh in (False, True):
        gs = _scene(pkg, sc, c1, lens, quads, normals, move, bvh)
        before, tables = _one_shot(torch, gs), _tables(gs)

        def refused(needle, arr=None, n=None, flags=0):
            arr = np.ascontiguousarray(arr if arr is not None else move)
            with pytest.raises(pkg.host.RtError) as e:
                pkg.hip._check(L.rt_hip_scene_set_flat_motion(gs._h, arr.ctypes.data, len(arr) if n is None else n, flags), L)
            assert e.value.code == abi.RT_ERR_INVALID and needle in str(e.value), str(e.value)
            assert _tables(gs) == tables
            _frames_equal(_one_shot(torch, gs), before, needle)
        bad = move.copy(); bad[40, 1] = np.nan; bad[60, 0] = np.inf
        refused("quad 40:", bad)
        bad = move.copy(); bad[7, 2] = -np.inf; bad[3, 0] = 1.7e308; bad[3, 1] = 1.7e308
        refused("quad 7:", bad)                                # (q + m of entry 3 is finite: 1.7e308 + a coordinate of order 1)
        refused("n_quads", move[:-1])
        refused("unknown flag", flags=4)
        refused("unknown flag", flags=abi.RT_UPDATE_FLATS_REBUILD)
        gs.close()
    with pytest.raises(pkg.host.RtError):
        pkg.hip._check(L.rt_hip_scene_set_flat_motion(None, None, 0, 0), L)
    # q + m: finite each, not finite together
    far = _with_geometry(quads, np.where(np.arange(9)[None, :] == 0, 1e308, _quv(quads)))
    gs = _scene(pkg, sc, c1, lens, far, None, None, False)
    bad = np.zeros((len(quads), 3)); bad[9, 0] = 1e308; bad[4, 0] = 1e308
    with pytest.raises(pkg.host.RtError) as e:
        gs.set_flat_motion(bad)
    assert "quad 4:" in str(e.value) and gs.query("flat_motion") == 0
    gs.close()


@pytest.mark.gpu
def test_headline_scene_keeps_its_kernel(pkg, load_scene, torch_cuda):
    sc = load_scene("cover", 48, 32, 2)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    _one_shot(torch, gs)
    assert gs.query("last_kernel") == 3 and gs.query("flat_motion") == 0 and gs.table("flat_motion") == b""
    with pytest.raises(pkg.host.RtError):
        gs.set_flat_motion(np.zeros((1, 3)))              # no flat primitive
    gs.close()


# ------------------------------------------------------------------ the CLI
@pytest.mark.gpu
def test_cli_renders_the_example_with_its_motion(pkg, abi, host, torch_cuda, tmp_path):
    """a 48 x 32 cut of scenes/make_flat_motion_scene.py through `raytracer`: the API frame of the same file byte for byte, and NOT the
    frame of the file with "move" stripped"""
    from PIL import Image
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_flat_motion_scene", os.path.join(ROOT, "scenes", "make_flat_motion_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = json.loads(mod.make(1))
    cfg.update(width=W, height=H, samples_per_pixel=SPP, max_depth=8)
    assert sum("move" in o for o in cfg["objects"]) == 2
    still_cfg = json.loads(json.dumps(cfg))
    for o in still_cfg["objects"]:
        o.pop("move", None)
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    imgs = {}
    for name, c in (("moving", cfg), ("still", still_cfg)):
        (tmp_path / f"{name}.json").write_text(json.dumps(c))
        r = subprocess.run([EXE, str(tmp_path / f"{name}.json"), str(tmp_path / f"{name}.png")], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.stdout, r.stderr)
        imgs[name] = np.asarray(Image.open(tmp_path / f"{name}.png").convert("RGB"))
    assert not np.array_equal(imgs["moving"], imgs["still"]), "the CLI ignored the file's motion"
    sc = host.Scene.load(str(tmp_path / "moving.json"))
    assert sc.flat_bvh() and sc.flat_motion() is not None
    gs = _scene(pkg, sc, quads=sc.quads(), normals=sc.flat_normals(), move=sc.flat_motion(), bvh=True)
    api, _ = gs.render_to_host()
    gs.close()
    assert np.array_equal(api, imgs["moving"])
