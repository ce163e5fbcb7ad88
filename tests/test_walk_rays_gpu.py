"""The device grid walk on adversarial rays, against brute force.

Every image depends on the walk picking the (t, sphere) that the reference's object-order scan picks (raytracer.rs:44-59).  The
CPU tests check that on adversarial rays through tests/hostsim — a g++ build of rt_core.h's per-lane hit_world_grid — but the
GPU runs other arithmetic (v_rcp_f32, v_med3_f32, minNum / maxNum) and, in the megakernel, another walk: the lock-step wave
form of rt_kernel.hip (two cells per round, the speculative second cell, the early stop, the `last` mailbox; packed and wide
tables).  Here the rays of tests/adversarial_rays.py go through both on the device:
  - rt_hip_render_rays_probe (librt_hip_probe.so): the real megakernel renders a W x H frame whose camera rays are the
    adversarial ones.  Sample 0's camera segment records what hit_world returned: it must equal a numpy brute force of
    Sphere::hit (sphere.rs:46-58) bit for bit; the whole frame must equal rt_oracle_render_rays within tests/parity.py's bar
    and trace the oracle's segments;
  - rt_hip_walk_probe: the device build of hit_world_grid, one ray per thread, must equal its host build bit for bit, and take
    the same number of grid steps and exact tests;
  - the worlds reach LDS, L2 and wide tables, unlit and lit (rt_hip_scene_query("last_kernel"), asserted by the last test).
Frames of the PRODUCT library cover its own code object: cameras whose every ray lies in a plane between cells."""
import ctypes as C
import json
import os

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

from adversarial_rays import (ALL_KINDS, FAMILIES, adversarial_world, brute_force_hit_world, grid_geometry, hit_world_v,
                              ray_table, sphere_arrays, sphere_hit_t)
from conftest import dvec
from fuzz_worlds import big_flat_world_json, fuzz_world_json
from parity import assert_parity, pooled_atol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")
W, H, SPP, DEPTH = 64, 48, 2, 5                  # a frame of 3 072 rays per world
HL, LDS, WIDE = 4, 1, 8
SEEN = {}                                       # (lit, table form) -> the world that ran it
COUNT = {"rays": 0, "hits": 0}
LIGHT = {"center": {"x": 0.0, "y": 30.0, "z": 10.0}, "radius": 8.0, "material": {"Light": {}}}

# (world, lit, environment): adversarial worlds 0-4 of tests/adversarial_rays.py, world 4 with thin cells (RT_GRID_N), world 1
# through the wide tables (RT_GRID_WIDE), a 5 000-sphere flat world whose tables stay in L2, and the fuzz worlds (two lights each)
CASES = ([(f"adv{wi}", wi % 2 == 1, {}) for wi in range(5)]
         + [("adv4", True, {"RT_GRID_N": "60,4,60"}), ("adv1", False, {"RT_GRID_WIDE": "1"}), ("adv1", True, {"RT_GRID_WIDE": "1"}),
            ("flat5000", False, {}), ("flat5000", True, {})]
         + [(f"fuzz{k}", True, {}) for k in range(6)])


def _case_id(case):
    world, lit, env = case
    return "-".join([world, "lit" if lit else "unlit"] + [f"{k}={v}" for k, v in env.items()])


def _materials(abi, spheres, n, rng, lit):
    """give the random worlds' spheres mixed materials (paths that bounce, refract and reach the sky) and, lit, one light"""
    for i in range(n):
        u = rng.random()
        spheres[i].kind = abi.RT_MAT_LAMBERTIAN if u < 0.55 else (abi.RT_MAT_METAL if u < 0.8 else abi.RT_MAT_GLASS)
        spheres[i].albedo[:] = [float(x) for x in rng.uniform(0.2, 0.95, 3)]
        spheres[i].fuzz_or_ior = float(rng.uniform(0.0, 0.5)) if spheres[i].kind == abi.RT_MAT_METAL else 1.5
    if lit:
        spheres[3].kind = abi.RT_MAT_LIGHT


class _World:
    """a scene (host struct, pointer for the C calls), its spheres, and the rays of one frame (H x W x 6)"""

    def __init__(self, abi, host, hostsim, world, lit, seed):
        rng = np.random.default_rng(seed)
        self.keep = None
        if world.startswith("adv"):
            sc, spheres, n = adversarial_world(abi, rng, int(world[3:]))
            _materials(abi, spheres, n, np.random.default_rng(seed + 1), lit)
            sc.sky_mode = abi.RT_SKY_GRADIENT
            self.keep, self.c, self.ptr = (sc, spheres), sc, C.pointer(sc)
            self.spheres, self.n_all, n_aim = spheres, sc.n_spheres, n
        else:
            if world == "flat5000":
                cfg = json.loads(big_flat_world_json(5000, np.random.default_rng(11), half=35.0))
                if lit:
                    cfg["objects"].append(LIGHT)
            else:
                cfg = json.loads(fuzz_world_json(np.random.default_rng(int(world[4:]) + 100), int(world[4:])))
            self.keep = host.Scene.loads(json.dumps(cfg))
            self.c, self.ptr = self.keep.c, self.keep.ptr
            self.spheres, self.n_all = self.c.spheres, self.c.n_spheres
            n_aim = self.n_all
        self.c.width, self.c.height, self.c.samples_per_pixel, self.c.max_depth = W, H, SPP, DEPTH
        self.grid = grid_geometry(hostsim, self.ptr)
        rays, self.fam = ray_table(rng, self.spheres, n_aim, W * H, tuple(range(ALL_KINDS)), self.grid)
        self.rays = rays.reshape(H, W, 6)
        self.centres, self.radii = sphere_arrays(self.spheres, self.n_all)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def test_brute_force_restatement_equals_the_oracle_sphere_hit(oracle, abi, hostsim):
    """the numpy Sphere::hit of these tests against the oracle's, pair by pair (tangents, rays from inside, far origins, negative
    radii), and its world-wide scan against tests/hostsim's brute force"""
    rng = np.random.default_rng(3)
    L = oracle.lib(abi)
    sc, spheres, n = adversarial_world(abi, rng, 0)
    rays, fam = ray_table(rng, spheres, n, 3000, tuple(range(FAMILIES)))
    centres, radii = sphere_arrays(spheres, sc.n_spheres)
    bb, tb = brute_force_hit_world(rays, centres, radii)
    pick = np.where(bb >= 0, bb, rng.integers(0, sc.n_spheres, len(rays)))   # (the sphere each ray hits first, if any)
    pick[::3] = rng.integers(0, sc.n_spheres, len(pick[::3]))
    got = np.concatenate([np.diagonal(sphere_hit_t(rays[k:k + 250, :3], rays[k:k + 250, 3:], centres[pick[k:k + 250]], radii[pick[k:k + 250]]))
                          for k in range(0, len(rays), 250)])
    out = (C.c_double * 10)()
    n_hit = 0
    for k in range(len(rays)):
        hit = L.rt_oracle_sphere_hit(dvec(*centres[pick[k]]), float(radii[pick[k]]), dvec(*rays[k, :3]), dvec(*rays[k, 3:]), 0.001,
                                     np.finfo(np.float64).max, out)
        want = out[0] if hit else np.inf
        assert got[k] == want, (k, fam[k], got[k], want)
        n_hit += bool(hit)
    assert n_hit > 1000, n_hit
    _, _, hb, ht = hit_world_v(hostsim, C.byref(sc), rays)
    assert (bb == hb).all() and (tb == ht).all()


def _frame_equal(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_walk_on_adversarial_rays(pkg, abi, host, hostsim, oracle, torch_cuda, monkeypatch, case):
    world, lit, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wd = _World(abi, host, hostsim, world, lit, seed=1000 + CASES.index(case))
    what = _case_id(case)
    gs = pkg.hip.HipScene(wd.ptr, 0, library=pkg.hip.probe_lib())
    try:
        rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def ordinary():
            gs.render(rgb.data_ptr(), lin.data_ptr(), None, stream)
            gs.wait()
            return rgb.cpu().numpy().copy(), lin.cpu().numpy().copy()
        before = ordinary()

        d_rays = _dev(wd.rays)
        first_t = torch.full((H, W), float("nan"), dtype=torch.float64, device="cuda:0")
        first_b = torch.full((H, W), -2, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        st = gs.render_rays_probe(d_rays.data_ptr(), rgb.data_ptr(), lin.data_ptr(), first_t.data_ptr(), first_b.data_ptr())
        key = gs.query("last_kernel")
        g_rgb, g_lin = rgb.cpu().numpy().copy(), lin.cpu().numpy().copy()
        p_t, p_b = first_t.cpu().numpy().reshape(-1), first_b.cpu().numpy().reshape(-1)

        # the device's per-lane walk (hit_world_grid) on the same rays
        n = W * H
        w_t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        w_b = torch.full((n,), -2, dtype=torch.int32, device="cuda:0")
        w_work = torch.full((n, 2), -1, dtype=torch.int32, device="cuda:0")
        gs.walk_probe(d_rays.data_ptr(), w_t.data_ptr(), w_b.data_ptr(), n, w_work.data_ptr(), stream)
        torch.cuda.synchronize()
        w_t, w_b, w_work = w_t.cpu().numpy(), w_b.cpu().numpy(), w_work.cpu().numpy().view(np.uint32)

        after = ordinary()
        assert _frame_equal(before, after), f"{what}: the probe frame changed the next ordinary frame"
    finally:
        gs.close()

    assert (key & HL != 0) == lit, (what, key)
    form = "wide" if key & WIDE else ("lds" if key & LDS else "l2")
    if "RT_GRID_WIDE" in env:
        assert form == "wide", (what, key)
    if world == "flat5000":
        assert form == "l2", (what, key)
    SEEN.setdefault((lit, form), what)

    rays = wd.rays.reshape(-1, 6)
    bb, tb = brute_force_hit_world(rays, wd.centres, wd.radii)
    h_work = np.zeros((n, 2), np.uint32)
    hg_b, hg_t, hb_b, hb_t = hit_world_v(hostsim, wd.ptr, rays, h_work)
    assert (hb_b == bb).all() and (hb_t == tb).all(), f"{what}: the numpy brute force and hostsim's disagree"

    def check(b, t, who):
        bad = np.flatnonzero((b != bb) | ((bb >= 0) & (t.view(np.int64) != tb.view(np.int64))))
        assert bad.size == 0, (f"{what}: {who} differs from brute force on {bad.size} of {n} rays; first: families {wd.fam[bad[:4]].tolist()} "
                               f"rays {rays[bad[:4]].tolist()} got {b[bad[:4]].tolist()} {t[bad[:4]].tolist()} want {bb[bad[:4]].tolist()} {tb[bad[:4]].tolist()}")
    # (1) the megakernel's first hit of every pixel, exactly
    check(p_b, p_t, "the megakernel's first hit")
    # (2) the device's per-lane walk equals its host build bit for bit (isolates v_rcp_f32 / v_med3_f32 from the wave form)
    assert (w_b == hg_b).all() and (w_t.view(np.int64) == hg_t.view(np.int64)).all(), f"{what}: device hit_world_grid != host build"
    # ... and takes the same walk: the same cells stepped through and the same spheres tested.  The device's v_rcp_f32 and
    # v_med3_f32 only move crossing times by an ulp, far inside the margins (GridDesc.pull, grid_begin's slack) that make the walk
    # conservative; a margin that is lost or shrunk shows here as walks of another length long before a hit goes missing.
    bad = np.flatnonzero((w_work != h_work).any(axis=1))
    assert bad.size == 0, (f"{what}: the device walk differs from the host build's on {bad.size} of {n} rays; first: families "
                           f"{wd.fam[bad[:4]].tolist()} device {w_work[bad[:4]].tolist()} host {h_work[bad[:4]].tolist()}")
    check(w_b, w_t, "the device's hit_world_grid")

    # (3) whole paths against the oracle through the same camera rays
    o_rgb, o_lin, o_st = oracle.render_rays(abi, wd.ptr, wd.rays)
    nan_g, nan_o = np.isnan(g_lin), np.isnan(o_lin)
    assert (nan_g == nan_o).all(), f"{what}: NaN pixels differ"
    assert_parity(g_rgb, np.where(nan_g, 0.0, g_lin), o_rgb, np.where(nan_o, 0.0, o_lin), what, atol=pooled_atol(SPP))
    assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (what, st["segments"], o_st["segments"], o_st["segments_discarded"])
    COUNT["rays"] += n
    COUNT["hits"] += int((bb >= 0).sum())
    assert (bb >= 0).sum() > 0.2 * n, (what, int((bb >= 0).sum()))


def _plane_camera(grid, ax, j, back):
    """a camera whose every ray lies in the plane x[ax] = gmin[ax] + j * size[ax]: origin on it, lower_left / horizontal / vertical
    with a zero component along ax (so every direction's ax component is exactly 0); it looks along the next axis from `back`
    cells before the grid and fans over the third"""
    gmin, size, ncell = grid
    b, c = (ax + 1) % 3, (ax + 2) % 3
    o = np.zeros(3)
    o[ax] = gmin[ax] + j * size[ax]
    o[b] = gmin[b] - back * size[b]
    o[c] = gmin[c] + 0.5 * ncell[c] * size[c]
    span_b, span_c = ncell[b] * size[b], ncell[c] * size[c]
    fwd, hor, ver = np.zeros(3), np.zeros(3), np.zeros(3)
    fwd[b] = span_b
    hor[c] = 1.2 * span_c
    ver[b] = 0.5 * span_b
    ll = o + fwd - 0.5 * hor
    cam = (o.tolist(), ll.tolist(), hor.tolist(), ver.tolist())
    assert cam[1][ax] == cam[0][ax] and cam[2][ax] == 0.0 and cam[3][ax] == 0.0
    return cam


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["lds", "l2"])
@pytest.mark.parametrize("lit", [False, True], ids=["unlit", "lit"])
def test_product_frames_on_cell_plane_cameras(pkg, abi, host, hostsim, oracle, torch_cuda, table, lit):
    """librt_hip.so itself (not the probe build): frames whose every camera ray lies in a plane between cells, against the
    oracle through the same camera"""
    from test_gpu_parity import _oracle_with_camera
    w, h, spp, depth = 48, 32, 4, 8
    if table == "l2":
        cfg = json.loads(big_flat_world_json(5000, np.random.default_rng(11), width=w, height=h, spp=spp, depth=depth, half=35.0))
    else:
        with open(COVER) as f:
            cfg = json.load(f)
        cfg.update(width=w, height=h, samples_per_pixel=spp, max_depth=depth)
    if lit:
        cfg["objects"].append(LIGHT)
    sc = host.Scene.loads(json.dumps(cfg))
    grid = grid_geometry(hostsim, sc.ptr)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    try:
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        for ax in range(3):
            for j in (int(grid[2][ax]) // 2, 1):
                cam = _plane_camera(grid, ax, j, back=3.0)
                gs.set_camera(*cam)
                gs.render(rgb.data_ptr(), lin.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
                st = gs.wait()
                key = gs.query("last_kernel")
                assert (key & HL != 0) == lit and (key & LDS != 0) == (table == "lds") and not key & WIDE, key
                o_rgb, o_lin, o_st = _oracle_with_camera(oracle, abi, sc, cam)
                what = f"{table} {'lit' if lit else 'unlit'} plane axis {ax} cell {j}"
                assert_parity(rgb.cpu().numpy(), lin.cpu().numpy(), o_rgb, o_lin, what, atol=pooled_atol(spp))
                assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (what, st["segments"], o_st["segments"])
    finally:
        gs.close()


@pytest.mark.gpu
def test_every_walk_path_ran():
    """the adversarial frames above reached the packed tables in LDS and in L2 and the wide tables, each unlit and lit"""
    want = {(lit, form) for lit in (False, True) for form in ("lds", "l2", "wide")}
    assert want <= set(SEEN), f"not covered: {sorted(want - set(SEEN))}; seen {SEEN}"
    print(f"adversarial rays checked on the device: {COUNT['rays']} ({COUNT['hits']} hits)")
