"""The structure over the flat primitives on the device: a scene created with it renders, in every bit, the frame of the
same scene created without it and of its own full scan ("variant" 1); the device form of the traversal through rt_hip_quad_probe against
the host build of the scan; worlds past the old cap; ties; the plumbing.  The unmarked tests check the inputs on the host build."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

import flat_bvh_rays as R
import flat_bvh_sim as F
import lane_sim
from quad_rays import T_MAX
from test_medium_gpu import _cfg, _lam, _load, _obj, _one_shot, _same, _stream
from test_quad_gpu import GLASS, _floor_objs, _hip_scene, _metal, _room_objs
from test_tri_gpu import TETRA, _mesh, parity_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 48, 32, 4
QUADS, ACCUM = 512, 16
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _sim():
    from conftest import graft
    return F.load(graft.load_package().abi)


# ------------------------------------------------------------------ worlds
def _make_bvh_scene():
    import importlib.util
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scenes"))
    try:
        spec = importlib.util.spec_from_file_location("make_bvh_scene", os.path.join(ROOT, "scenes", "make_bvh_scene.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scenes"))
    return mod


def _icosphere(c, r, subdivision):
    v, f = _make_bvh_scene().icosphere(c, r, subdivision)
    return [[round(x, 3) for x in p] for p in v], f


def _example_cfg():
    """the example scene (scenes/cornell_icosphere_600x600_spp128.json as scenes/make_bvh_scene.py writes it)"""
    return json.loads(_make_bvh_scene().make())


# six small worlds (the first at two depths): every one holds more than four flat primitives, so its structure has inner nodes
FRAME_CASES = [("tetra", 8), ("tetra", 50), ("room_glass", 8), ("metal_ico", 8), ("lens_moving", 8), ("medium", 8), ("solid", 8)]


def frame_cfg(case):
    if case == "room_glass":      # the lit room with an 80-face icosphere in Glass where its box stood
        objs = _room_objs()
        at = [i for i, o in enumerate(objs) if "box" in o]
        objs[at[0]] = _mesh(*_icosphere((-0.8, -0.3, -0.7), 0.6, 1), GLASS)
        return _cfg(objs, sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0))
    if case == "metal_ico":       # a Metal icosphere (20 faces) beside the spheres
        return _cfg(_floor_objs(extra=[_mesh(*_icosphere((-1.2, 0.6, 2.4), 0.9, 0), _metal((0.9, 0.9, 0.9), 0.0))]))
    if case == "solid":           # Checker and Noise triangles (and a tetrahedron: more than four flat primitives)
        cfg = parity_cfg(case)
        cfg["objects"].append(_mesh(*TETRA, _lam(0.3, 0.7, 0.4)))
        return cfg
    return parity_cfg(case)       # tests/test_tri_gpu.py: floor + tetrahedron + spheres; lens + moving spheres; a Medium cut by a triangle; solids


def frame_world(host, case, depth):
    sc, c1, lens = _load(host, frame_cfg(case), W, H, SPP, depth, seed=71 + depth)
    return sc, c1, lens, sc.quads()


def _bvh_scene(pkg, sc, c1=None, lens=None, quads=None, library=None):
    gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=c1, quads=quads, flat_bvh=True)
    if lens:
        gs.set_lens(*lens)
    return gs


def test_frame_worlds_have_inner_nodes(host, abi):
    sim = _sim()
    for case, depth in FRAME_CASES:
        sc, c1, lens, quads = frame_world(host, case, depth)
        nodes, order, n_always = sim.build(quads)
        assert len(quads) > 4 and nodes["count"][0] == 0 and n_always == 0, case


@pytest.mark.gpu
@pytest.mark.parametrize("case,depth", FRAME_CASES)
def test_frames_with_the_structure_equal_the_scan(pkg, abi, host, torch_cuda, case, depth):
    """created both ways: linear radiance, RGB8 and segments equal bit for bit, and equal to "variant" 1 on the structure scene; the AOVs and
    the surface record equal bitwise on two of the worlds"""
    sc, c1, lens, quads = frame_world(host, case, depth)
    plain = _hip_scene(pkg, sc, c1, lens, quads)
    want = _one_shot(torch, plain)
    gs = _bvh_scene(pkg, sc, c1, lens, quads)
    assert plain.query("flat_bvh") == 0 and gs.query("flat_bvh") > 1 and gs.query("quads") == len(quads)
    got = _one_shot(torch, gs)
    k = gs.query("last_kernel")
    assert k == plain.query("last_kernel") and k & QUADS
    _same(want, got, f"{case}: structure vs scan")
    assert got[2]["segments"] == want[2]["segments"] > 0
    gs.set_option("variant", 1)
    brute = _one_shot(torch, gs)
    gs.set_option("variant", 0)
    _same(got, brute, f"{case}: variant 1")
    assert brute[2]["segments"] == got[2]["segments"]
    if case in ("tetra", "medium") and depth == 8:
        for scene in (plain, gs):
            scene._aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
            scene._surf = torch.zeros((H, W, 2), dtype=torch.float64, device="cuda:0")
            scene.render_aovs(SPP, scene._aov.data_ptr(), None, _stream(torch))
            scene.render_surface(scene._surf.data_ptr(), None, _stream(torch))
        torch.cuda.synchronize()
        assert torch.equal(plain._aov.view(torch.int32), gs._aov.view(torch.int32)) and torch.equal(plain._surf.view(torch.int64), gs._surf.view(torch.int64))
        assert bool(plain._aov.any()) and bool((plain._surf.view(torch.int64) != 0).any())
    plain.close(); gs.close()


# ------------------------------------------------------------------ past the old cap
def _c_flats(abi, quvs, shapes, kind=0):
    return F.flats_array(abi, quvs, shapes, kind)


def _c_scene(abi, w, h, spp=SPP, depth=6, origin=(0.0, 9.0, 0.5), look=(-5.0, -5.0)):
    """one small sphere (id 0) above the origin; the camera looks down on the plane y = 0 (the square [-5, 5]^2)"""
    spheres = (abi.RtSphere * 1)()
    spheres[0].center[:] = [0.5, 1.2, 0.3]
    spheres[0].radius = 0.6
    spheres[0].albedo[:] = [0.6, 0.5, 0.7]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=w, height=h, samples_per_pixel=spp, max_depth=depth, sky_mode=abi.RT_SKY_GRADIENT, spheres=spheres,
                     n_spheres=1, seed=4711)
    sc.cam_origin[:] = list(origin)
    sc.cam_lower_left[:] = [look[0], 0.0, look[1]]; sc.cam_horizontal[:] = [10.0, 0.0, 0.0]; sc.cam_vertical[:] = [0.0, 0.0, 10.0]
    return sc, spheres


@functools.lru_cache(maxsize=None)
def _big_world(name):
    from test_flat_bvh_cpu import heightfield
    quv = heightfield()
    if name == "1025":
        quv = quv[np.random.default_rng(31).permutation(2048)[:1025]]
    quv.setflags(write=False)
    return quv


def _camera_rays(sc):
    """the pinhole rays of pixel centres (any rays do: the probe traces what it is given): h x w x 6"""
    w, h = sc.width, sc.height
    o = np.array(list(sc.cam_origin))
    u = (np.arange(w) + 0.5) / w
    v = (np.arange(h) + 0.5) / h
    tgt = np.array(list(sc.cam_lower_left))[None, None, :] + u[None, :, None] * np.array(list(sc.cam_horizontal)) + v[:, None, None] * np.array(list(sc.cam_vertical))
    return np.concatenate([np.broadcast_to(o, tgt.shape), tgt - o], axis=2)


def surface_rays(sc):
    """the pixel-centre pinhole rays of the surface record, row by row: (h w) x 6"""
    w, h = sc.width, sc.height
    o = np.array(list(sc.cam_origin))
    u = (np.arange(w) + 0.5) / (w - 1)
    v = (h - (np.arange(h) + 0.5)) / (h - 1)
    tgt = np.array(list(sc.cam_lower_left))[None, None, :] + u[None, :, None] * np.array(list(sc.cam_horizontal)) + v[:, None, None] * np.array(list(sc.cam_vertical))
    return np.concatenate([np.broadcast_to(o, tgt.shape), tgt - o], axis=2).reshape(-1, 6)


def walk_witness(sim, flats, rays, id_base):
    """what the host build's walk does with each ray alone, from its counters: the root's count (0: an inner node), the always-visited
    entries, and the number of rays rejected at the root (one box test, no entry test), of rays that reach an entry test in a leaf, and
    of rays that take the out-of-range fallback"""
    nodes, order, n_always = sim.build(flats)
    at_root = in_leaf = fallback = 0
    for r in rays:
        _, _, cnt = sim.hit(flats, r[None, :], np.array([T_MAX]), True, id_base)
        assert cnt["rays_bvh"] + cnt["rays_scan"] == 1
        at_root += cnt["rays_bvh"] == 1 and cnt["box_tests"] == 1 and cnt["entry_tests"] == 0
        in_leaf += cnt["rays_bvh"] == 1 and cnt["entry_tests"] > 0
        fallback += cnt["rays_scan"]
    return dict(nodes=len(nodes), root_count=int(nodes["count"][0]), n_always=n_always, at_root=int(at_root), in_leaf=int(in_leaf), fallback=int(fallback))


@pytest.mark.parametrize("name", ["1025", "2048"])
def test_big_worlds_on_the_host_build(abi, name):
    quv = _big_world(name)
    sim = _sim()
    sc, keep = _c_scene(abi, W, H)
    rays = _camera_rays(sc).reshape(-1, 6)
    flats = _c_flats(abi, quv, 1)
    b0, t0, _ = sim.hit(flats, rays, np.full(len(rays), T_MAX), False, 1)
    b1, t1, cnt = sim.hit(flats, rays, np.full(len(rays), T_MAX), True, 1)
    assert np.array_equal(b0, b1) and np.array_equal(_bits(t0), _bits(t1)) and cnt["rays_scan"] == 0
    assert (b0 >= 1).mean() > (0.25 if name == "1025" else 0.5) and len(np.unique(b0)) > 200


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1025", "2048"])
def test_past_the_old_cap(pkg, abi, torch_cuda, name):
    """1 025 triangles and a 32 x 32 heightfield of 2 048: refused without the structure; the frame equals its "variant" 1 frame bit for bit;
    rt_hip_render_rays_probe's sample-0 (t, id) equals the host build's scan behind the sphere"""
    from test_quad_rays_gpu import _frames_of_both_variants
    quv = _big_world(name)
    flats = _c_flats(abi, quv, 1)
    sc, keep = _c_scene(abi, W, H)
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(C.pointer(sc), 0, quads=flats)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=flats, flat_bvh=True)
    try:
        assert gs.query("quads") == len(quv) and gs.query("flat_bvh") > len(quv) // 4
        a = _one_shot(torch, gs)
        gs.set_option("variant", 1)
        b = _one_shot(torch, gs)
        gs.set_option("variant", 0)
        _same(a, b, "variant 1")
        assert a[2]["segments"] == b[2]["segments"] and gs.query("last_kernel") & QUADS
        rays = _camera_rays(sc)
        (_, _, _), p_t, p_b, _ = _frames_of_both_variants(gs, rays, W, H, name)
    finally:
        gs.close()
    # the host build: the sphere first (lane simulator), then the scan over the flat primitives
    lanes = lane_sim.load(abi)
    rc, best, t, _ = lanes.hit_world_v(sc, rays.reshape(-1, 6), quads=flats)
    assert rc == 0
    bad = np.flatnonzero((p_b != best) | ((best >= 0) & (_bits(p_t) != _bits(t))))
    assert bad.size == 0, (bad[:5], p_b[bad[:5]], best[bad[:5]])
    assert (best >= 1).sum() > 0.3 * len(best) and (best == 0).sum() > 0


# ------------------------------------------------------------------ the device form through rt_hip_quad_probe
PROBE_GATHERED = ["generic", "edges", "hypotenuse", "t_range", "non_finite", "magnitudes"]
PROBE_NEW = ["box_faces", "zero_components", "flat_walls"]


@functools.lru_cache(maxsize=None)
def _probe_table(cls):
    from conftest import graft
    abi = graft.load_package().abi
    table = R.gathered(cls, lane_sim.load(abi)) if cls in PROBE_GATHERED else R.new_class(cls, _sim(), abi)
    for a in table:
        a.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def _probe_reference(cls, first=0, count=None):
    """the host build's SCAN of entries first .. first + count - 1 of the class's list (ids from 1: one sphere in front) and the record"""
    from conftest import graft
    abi = graft.load_package().abi
    sim = _sim()
    quvs, shapes, rays, closest = _probe_table(cls)
    count = len(quvs) - first if count is None else count
    flats = _c_flats(abi, quvs[first:first + count], shapes[first:first + count])
    with np.errstate(all="ignore"):
        best, t, _ = sim.hit(flats, rays, closest, False, 1 + first)
        P, nrm, front = sim.surface(flats, rays, best, t, 1 + first)
    t = np.where(best >= 0, t, 0.0)
    return best, t, P, nrm, front


@pytest.mark.parametrize("cls", PROBE_GATHERED + PROBE_NEW)
def test_probe_tables_on_the_host_build(cls):
    quvs, shapes, rays, closest = _probe_table(cls)
    best = _probe_reference(cls)[0]
    print(f"{cls}: {int((best >= 0).sum())} of {len(rays)} rays hit (host build, scan)")
    assert len(rays) >= 100_000 and len(quvs) >= 100 and (len(rays) - 3) % 64 != 0
    assert (best >= 0).sum() > (0 if cls in ("magnitudes", "non_finite") else 0.02 * len(rays))


def _probe_run(pkg, abi, cls, first, count, n_rays):
    from test_quad_rays_gpu import _ProbeOut, _dev
    from test_tri_gpu import _probe_scene
    quvs, shapes, rays, closest = _probe_table(cls)
    flats = _c_flats(abi, quvs, shapes)
    spheres = (abi.RtSphere * 1)()
    spheres[0].center[:] = [0.0, 0.0, -60.0]
    spheres[0].radius = 0.5
    spheres[0].albedo[:] = [0.6, 0.5, 0.7]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=2, max_depth=5, sky_mode=abi.RT_SKY_GRADIENT, spheres=spheres, n_spheres=1,
                     seed=4242)
    sc.cam_origin[:] = [0.0, 0.0, 30.0]; sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]; sc.cam_horizontal[:] = [3.0, 0.0, 0.0]; sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=flats, flat_bvh=True)
    try:
        assert gs.query("flat_bvh") > 1 and gs.query("quads") == len(quvs)
        d_rays, d_closest = _dev(rays[:n_rays]), _dev(closest[:n_rays])
        out = _ProbeOut(n_rays)
        gs.quad_probe(d_rays.data_ptr(), d_closest.data_ptr(), n_rays, first, count, *out.ptrs(0), stream=_stream(torch))
        torch.cuda.synchronize()
        return out.fetch()
    finally:
        gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", PROBE_GATHERED + PROBE_NEW)
def test_device_traversal_equals_the_host_scan(pkg, abi, torch_cuda, cls):
    """the full range of a structure scene — the device form of flats_hit_bvh, one launch of all the class's rays but the last 3 (not a
    multiple of 64: the last wave walks under a partial exec mask) — against the host build's SCAN: accept, t, P, normal, front_face"""
    from test_quad_rays_gpu import _assert_probe_equals
    quvs, shapes, rays, closest = _probe_table(cls)
    n = len(rays) - 3
    assert n % 64 != 0 and n >= 99_997
    got = _probe_run(pkg, abi, cls, 0, len(quvs), n)
    best, t, P, nrm, front = (a[:n] for a in _probe_reference(cls))
    _assert_probe_equals(cls, got, best, t, P, nrm, front)
    print(f"{cls}: {int((best >= 0).sum())} of {n} rays hit (device, structure)")


@pytest.mark.gpu
def test_a_proper_sub_range_takes_the_scan_of_that_range(pkg, abi, torch_cuda):
    from test_quad_rays_gpu import _assert_probe_equals
    n = 20_001
    got = _probe_run(pkg, abi, "generic", 17, 40, n)
    best, t, P, nrm, front = (a[:n] for a in _probe_reference("generic", 17, 40))
    assert (best >= 0).sum() > 200 and best[best >= 0].min() >= 18 and best.max() <= 57
    _assert_probe_equals("sub-range", got, best, t, P, nrm, front)


# ------------------------------------------------------------------ ties through the megakernel
def _tie_row(abi):
    """the coincident-entries world of tests/test_flat_bvh_cpu.py under a one-row camera at x = -9 that looks into the overlap"""
    from test_flat_bvh_cpu import _tie_world
    quv, shapes = _tie_world()
    sc, keep = _c_scene(abi, 64, 1, spp=2, depth=4, origin=(-9.0, 0.0, 0.0))
    sc.cam_lower_left[:] = [0.0, 0.0, 0.1]; sc.cam_horizontal[:] = [0.0, 0.0, 1.8]; sc.cam_vertical[:] = [0.0, 0.0, 0.0]
    keep[0].center[:] = [0.0, 40.0, 0.0]
    return quv, shapes, sc, keep


def test_tie_row_on_the_host_build(abi):
    quv, shapes, sc, keep = _tie_row(abi)
    rays = _camera_rays(sc).reshape(-1, 6)
    flats = _c_flats(abi, quv, shapes)
    b, t, cnt = _sim().hit(flats, rays, np.full(len(rays), T_MAX), True, 1)
    assert (b == 1 + 1).all() and cnt["entry_tests"] == 8 * len(rays), "every camera ray meets both walls; the smaller index wins, visited second"


@pytest.mark.gpu
def test_ties_through_the_megakernel(pkg, abi, torch_cuda):
    """the coincident-entries world as a one-row frame: with the structure, without, and variant 1 — one frame; the first hit is the
    smaller index on every pixel"""
    from test_quad_rays_gpu import _frames_of_both_variants
    quv, shapes, sc, keep = _tie_row(abi)
    flats = _c_flats(abi, quv, shapes)
    plain = pkg.hip.HipScene(C.pointer(sc), 0, quads=flats)
    want = _one_shot(torch, plain)
    plain.close()
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=flats, flat_bvh=True)
    try:
        got = _one_shot(torch, gs)
        _same(want, got, "ties")
        assert got[2]["segments"] == want[2]["segments"]
        _, p_t, p_b, _ = _frames_of_both_variants(gs, _camera_rays(sc), 64, 1, "ties")
        assert (p_b == 2).all()
    finally:
        gs.close()


# ------------------------------------------------------------------ plumbing
@pytest.mark.gpu
def test_plumbing_on_one_structure_scene(pkg, abi, host, torch_cuda):
    from test_gpu_parity import _with_env
    sc, c1, lens, quads = frame_world(host, "tetra", 8)
    ref = _hip_scene(pkg, sc, None, None, quads)
    want = _one_shot(torch, ref)
    gs = _bvh_scene(pkg, sc, None, None, quads)
    sim = _sim()
    nodes_b, order_b = sim.scene_tables(sc.ptr, quads)
    assert gs.query("flat_bvh") == len(nodes_b) // 64 > 1 and gs.table("flat_bvh") == nodes_b and gs.table("flat_bvh_order") == order_b
    assert ref.query("flat_bvh") == 0 and ref.table("flat_bvh") == b"" and ref.table("flat_bvh_order") == b""
    assert set(pkg.hip.TABLES) >= {"flat_bvh", "flat_bvh_order"}
    one = _one_shot(torch, gs)
    assert gs.query("last_kernel") == QUADS
    _same(want, one, "structure vs scan")
    _same(one, _one_shot(torch, gs), "second render")
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
    assert gs.query("last_kernel") == QUADS | ACCUM
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    # adaptive at threshold 0: every tile takes every sample — the scan scene's frame
    a_rgb, a_spp, a_st = gs.render_adaptive(0.0, 2)
    r_rgb, r_spp, r_st = ref.render_adaptive(0.0, 2)
    assert np.array_equal(a_rgb, r_rgb) and np.array_equal(a_spp, r_spp) and a_st["segments"] == r_st["segments"]
    # moved spheres: the structure stays, byte for byte, and the frame is a fresh scene's
    n = sc.c.n_spheres
    c0 = np.array([list(sc.c.spheres[i].center) for i in range(n)])
    new = c0 + np.array([[0.3, 0.1, -0.2], [-0.1, 0.2, 0.3], [0.2, 0.0, 0.1], [0.0, 0.3, -0.3]])
    gs.update_spheres(new, None)
    moved = _one_shot(torch, gs)
    for i in range(n):
        sc.c.spheres[i].center[:] = new[i]
    fresh = _bvh_scene(pkg, sc, None, None, quads)
    _same(moved, _one_shot(torch, fresh), "updated vs fresh")
    for name in ("geom", "cell_word", "cell_items", "large", "quads", "quad_lim", "flat_bvh", "flat_bvh_order"):
        assert gs.table(name) == fresh.table(name), name
    assert gs.table("flat_bvh") == nodes_b
    gs.close(); fresh.close(); ref.close()
    # a group of 2 is one rank
    alone = _bvh_scene(pkg, sc, None, None, quads)
    frame, st = alone.render_to_host()
    alone.close()
    for world in (1, 2):
        grp = _with_env({"RT_GPUS_EMULATE": "1"}, lambda: pkg.hip.HipGroup(sc.ptr, world, quads=quads, flat_bvh=True))
        out, gst = grp.render_to_host()
        assert np.array_equal(out, frame) and gst["segments"] == st["segments"], world
        grp.close()


@pytest.mark.gpu
def test_refusals(pkg, abi, host, torch_cuda):
    sc, _, _ = _load(host, _cfg([_obj((0, 0, 0), 1.0, _lam(0.5, 0.5, 0.5))]), 8, 8, 1, 2)
    L = pkg.hip.lib()
    one = _c_flats(abi, [[-1.0, -1.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0, 0.0]], 1)
    h = C.c_void_p()
    # the count is checked before any record is read: RT_MAX_FLATS_BVH + 1 through a one-record array
    assert L.rt_hip_scene_create_flats_bvh(sc.ptr, None, one, abi.RT_MAX_FLATS_BVH + 1, 0, C.byref(h)) == abi.RT_ERR_UNSUPPORTED and not h
    assert L.rt_hip_group_create_flats_bvh(sc.ptr, None, one, abi.RT_MAX_FLATS_BVH + 1, 1, C.byref(h)) == abi.RT_ERR_UNSUPPORTED and not h
    assert L.rt_hip_scene_create_flats_bvh(sc.ptr, None, one, 0, 0, C.byref(h)) == abi.RT_ERR_INVALID and not h
    assert L.rt_hip_scene_create_flats_bvh(sc.ptr, None, None, 0, 0, C.byref(h)) == abi.RT_ERR_INVALID and not h
    assert L.rt_hip_group_create_flats_bvh(sc.ptr, None, one, 0, 1, C.byref(h)) == abi.RT_ERR_INVALID and not h
    assert L.rt_hip_scene_create_flats_bvh(sc.ptr, None, None, 3, 0, C.byref(h)) == abi.RT_ERR_INVALID and not h
    bad = _c_flats(abi, [[-1.0, -1.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0, 0.0]] * 2, [1, 2])
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0, quads=bad, flat_bvh=True)
    assert e.value.code == abi.RT_ERR_INVALID and "quad 1: bad shape" in str(e.value)
    # wide tables (more than 65 535 spheres) have no QUADS kernels, with or without the structure
    n = 65_536
    spheres = (abi.RtSphere * n)()
    grid = np.arange(n)
    for i in range(n):
        spheres[i].center[:] = [float(grid[i] % 256), 0.0, float(grid[i] // 256)]
        spheres[i].radius = 0.3
    wide = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=1, max_depth=2, sky_mode=abi.RT_SKY_GRADIENT, spheres=spheres, n_spheres=n,
                       seed=1)
    wide.cam_origin[:] = [0.0, 5.0, 30.0]; wide.cam_lower_left[:] = [-1.5, 4.0, 29.0]; wide.cam_horizontal[:] = [3.0, 0.0, 0.0]; wide.cam_vertical[:] = [0.0, 2.0, 0.0]
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(C.pointer(wide), 0, quads=one, flat_bvh=True)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED and "wide tables" in str(e.value)
    with pytest.raises(ValueError):
        pkg.hip.HipScene(sc.ptr, 0, flat_bvh=True)


@pytest.mark.gpu
def test_cli_on_a_cut_of_the_example(pkg, host, torch_cuda, tmp_path):
    """48 x 32 of scenes/cornell_icosphere_600x600_spp128.json: the file key, and --flat-bvh on the same file without the key and cut to
    1 024 entries... the two routes agree wherever both exist: here on the first 1 000 flat primitives of the example"""
    from PIL import Image
    cfg = _example_cfg()
    cfg.update(width=W, height=H, samples_per_pixel=4)
    # cut the Glass model to 995 faces and drop the Metal one: 5 walls + 995 triangles = 1 000 entries fit the scan too
    glass = cfg["objects"][6]
    glass["mesh"]["faces"] = glass["mesh"]["faces"][:995]
    cfg["objects"] = cfg["objects"][:7]
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    png = {}
    for name, key, flags in (("key", True, []), ("flag", False, ["--flat-bvh"]), ("scan", False, [])):
        c = dict(cfg)
        if key:
            c["flat_bvh"] = True
        else:
            c.pop("flat_bvh", None)
        p = tmp_path / f"{name}.json"
        p.write_text(json.dumps(c))
        r = subprocess.run([exe, str(p), str(tmp_path / f"{name}.png")] + flags, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and os.path.exists(tmp_path / f"{name}.png"), (name, r.stdout, r.stderr)
        png[name] = np.asarray(Image.open(tmp_path / f"{name}.png"))
    assert np.array_equal(png["key"], png["flag"]) and np.array_equal(png["key"], png["scan"]) and png["key"].any()
    assert len(np.unique(png["key"].reshape(-1, 3), axis=0)) > 50
    # and the library call on the file with the key
    c = dict(cfg); c["flat_bvh"] = True
    sc, c1, ln = _load(host, c)
    assert sc.flat_bvh() and len(sc.quads()) == 1000
    gs = _bvh_scene(pkg, sc, c1, ln, sc.quads())
    want = _one_shot(torch, gs)[0]
    gs.close()
    assert np.array_equal(png["key"], want)
