"""Solid textures on the GPU, through the C ABI: small frames against the restatement (tests/solid_mini.py), every one of
the 128 SOLID instantiations launched, composition with passes / row shards / repeated renders, the first-hit AOVs, and two checks that
are independent of every restatement: the pattern rides a moving sphere, and a fine checker averages to the mean of its colours."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import fuzz_worlds as FW
import solid_mini as SM
from parity import assert_parity, pooled_atol
from test_kernel_matrix import ALL_KEYS, CELLS, WIDE, _cell_id, _cell_json, _key
from test_medium_gpu import _cfg, _hip_scene, _lam, _load, _med, _obj, _one_shot, _same, _stream

SOLID, MEDIUM, MOTION, LENS, ACCUM = 256, 128, 64, 32, 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLID_SCENE = os.path.join(ROOT, "scenes", "cover_solid_1200x800_spp128.json")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _chk(even, odd, scale):
    return {"Checker": {"even": list(even), "odd": list(odd), "scale": scale}}


def _noi(albedo, scale, mode=None, octaves=None, seed=None):
    body = {"albedo": list(albedo), "scale": scale}
    for k, v in (("mode", mode), ("octaves", octaves), ("seed", seed)):
        if v is not None:
            body[k] = v
    return {"Noise": body}


def _unlit_objs(moving, medium=False):
    """checkered ground of radius 100; a marble, a noise and a turbulence sphere; a glass sphere in front of them; a negative-radius
    checker shell.  moving: the solid spheres move over the shutter.  medium: a ball of smoke around the noise sphere"""
    mv = (lambda c, d: tuple(a + b for a, b in zip(c, d))) if moving else (lambda c, d: None)
    objs = [
        _obj((0, -100.5, 0), 100.0, _chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 1.5)),
        _obj((0, 0.5, 0), 1.0, _noi((0.9, 0.85, 0.8), 2.0, "marble", 5, 7), mv((0, 0.5, 0), (0.3, 0.2, 0.0))),
        _obj((2.2, 0.3, 0.5), 0.8, _noi((0.3, 0.8, 0.9), 4.0), mv((2.2, 0.3, 0.5), (0.0, 0.15, 0.1))),
        _obj((-2.2, 0.3, 0.0), 0.8, _noi((0.9, 0.5, 0.2), 3.0, "turbulence", 3, 4294967295), mv((-2.2, 0.3, 0.0), (-0.2, 0.0, 0.3))),
        _obj((0.6, 0.0, 2.5), 0.5, {"Glass": {"index_of_refraction": 1.5}}),
        _obj((-1.0, -0.1, 2.2), -0.4, _chk((0.8, 0.2, 0.2), (0.1, 0.1, 0.7), 6.0), mv((-1.0, -0.1, 2.2), (0.1, 0.1, 0.0))),
    ]
    if medium:
        objs.append(_obj((2.2, 0.3, 0.5), 1.3, _med((0.8, 0.8, 0.8), 0.9)))
    return objs


def _lit_objs(moving, medium=False):
    """black sky, one Light, the checkered ground and a marble sphere"""
    mv = (lambda c, d: tuple(a + b for a, b in zip(c, d))) if moving else (lambda c, d: None)
    objs = [
        _obj((0, -100.5, 0), 100.0, _chk((0.9, 0.9, 0.9), (0.3, 0.3, 0.3), 2.0)),
        _obj((0, 4.0, 0), 1.0, {"Light": {}}),
        _obj((0, 0.5, 0), 1.0, _noi((0.9, 0.9, 0.7), 2.5, "marble"), mv((0, 0.5, 0), (0.4, 0.0, 0.2))),
        _obj((1.7, 0.0, 1.0), 0.5, _noi((0.2, 0.4, 0.8), 5.0, "turbulence", 2, 3), mv((1.7, 0.0, 1.0), (0.0, 0.2, 0.0))),
    ]
    if medium:
        objs.append(_obj((-1.5, 0.4, 0.8), 0.9, _med((0.9, 0.9, 0.9), 0.8)))
    return objs


def _mini(oracle, abi, sc, center1=None, lens=None):
    L = oracle.lib(abi)
    return SM.SolidMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), center1, lens)


LENS_KEYS = {"aperture": 0.25, "focus_dist": 6.0}
PARITY_CASES = [(world, variant, depth) for world in ("unlit", "lit") for variant, depth in
                (("plain", 8), ("plain", 50), ("lens", 8), ("moving", 8), ("lens_moving", 8), ("medium", 8))]
_MINI_CACHE = {}


def parity_world(host, world, variant, depth):
    """(host scene, center1, lens, spp, objects) of one parity case: 24 x 16 at spp 4"""
    moving, lens_on, medium = "moving" in variant, "lens" in variant, variant == "medium"
    objs = _unlit_objs(moving, medium) if world == "unlit" else _lit_objs(moving, medium)
    cfg = _cfg(objs, sky=world == "unlit", lens=LENS_KEYS if lens_on else None)
    sc, c1, lens = _load(host, cfg, 24, 16, 4, depth, seed=31 + depth)
    assert (c1 is not None) == moving and (lens is not None) == lens_on
    return sc, c1, lens, 4, objs


def mini_frame(oracle, abi, host, world, variant, depth):
    """SolidMini's frame of a parity case, computed once per session and left unchanged (the CPU and the GPU tests share it)"""
    key = (world, variant, depth)
    if key not in _MINI_CACHE:
        sc, c1, lens, _, _ = parity_world(host, world, variant, depth)
        m = _mini(oracle, abi, sc, c1, lens)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _MINI_CACHE[key] = (rgb, lin, segs, m.discarded)
    return _MINI_CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("world,variant,depth", PARITY_CASES)
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, world, variant, depth):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against SolidMini; last_kernel carries SOLID; the
    full scan gives the same frame bit for bit"""
    torch = torch_cuda
    sc, c1, lens, spp, objs = parity_world(host, world, variant, depth)
    gs = _hip_scene(pkg, sc, c1, lens)
    assert gs.query("solids") == sum("Checker" in o["material"] or "Noise" in o["material"] for o in objs)
    rgb, lin, st = _one_shot(torch, gs)
    k = gs.query("last_kernel")
    assert k & SOLID and bool(k & MOTION) == ("moving" in variant) and bool(k & LENS) == ("lens" in variant), k
    assert bool(k & 4) == (world == "lit") and bool(k & MEDIUM) == (variant == "medium"), k
    m_rgb, m_lin, m_segs, m_disc = mini_frame(oracle, abi, host, world, variant, depth)
    print(f"{world} {variant} depth {depth}: max |linear diff| {float(np.abs(lin - m_lin).max()):.3g}, segments gpu {st['segments']} mini {m_segs} - {m_disc}")
    assert_parity(rgb, lin, m_rgb, m_lin, f"{world} {variant}", atol=pooled_atol(spp))
    assert st["segments"] == m_segs - m_disc, (st["segments"], m_segs, m_disc)
    gs.set_option("variant", 1)
    b = _one_shot(torch, gs)
    _same((rgb, lin), b, "variant 1")
    assert b[2]["segments"] == st["segments"]
    gs.close()


# One scene per cell of the SOLID sweep, in the sweep's order: (lights, colour map, LDS / L2 tables) x pinhole / lens x static / moving x
# without / with media.
SWEEP_CELLS = [(hl, simple, form, with_lens, moving, medium) for hl, simple, form in CELLS if form != "wide"   # (solids with wide tables are
               for with_lens in (False, True) for moving in (False, True) for medium in (False, True)]         #  refused, below)
SWEEP_KEYS = {SOLID | me | m | l | k for k in ALL_KEYS if not k & WIDE for me in (0, MEDIUM) for m in (0, MOTION) for l in (0, LENS)}   # the 128


def sweep_name(cell):
    return _cell_id(cell[:3]) + ("/lens" if cell[3] else "") + ("/moving" if cell[4] else "") + ("/medium" if cell[5] else "")


def sweep_key(cell):
    """last_kernel of a cell's one-shot frame"""
    return SOLID | (MEDIUM if cell[5] else 0) | (MOTION if cell[4] else 0) | (LENS if cell[3] else 0) | _key(*cell[:3])


def sweep_world(host, cell, width, height, pinhole=False):
    """(host scene, center1, lens, number of solids, number of media) of one cell at width x height, spp 2: the cell's world of
    test_kernel_matrix.py with a checkered ground and every third sphere a Noise; medium: another third are media; moving: every second
    sphere moves over the shutter.  pinhole: the same world without the cell's lens."""
    hl, simple, form, with_lens, moving, medium = cell
    cfg = json.loads(_cell_json(hl, simple, form, width=width, height=height, spp=2))
    rng = np.random.default_rng(2 * SWEEP_CELLS.index(cell))
    n_solids = n_media = 0
    for i, o in enumerate(cfg["objects"]):
        if "Light" in o["material"]:
            continue
        if i == 0:   # the ground keeps its colour (the general colour map's albedo above 1 included) as a checker
            a = next(iter(o["material"].values())).get("albedo", [0.5, 0.5, 0.5])
            o["material"] = _chk(a, [0.1, 0.1, 0.1], 2.0)
            n_solids += 1
        elif i % 3 == 1:
            o["material"] = _noi([0.8, 0.7, 0.6], 3.0, ("noise", "turbulence", "marble")[i % 9 // 3], 1 + i % 4, i)
            n_solids += 1
        elif medium and i % 3 == 2 and o["radius"] > 0:
            o["material"] = _med([0.8, 0.7, 0.6], round(float(rng.uniform(1.0, 10.0)), 3))
            n_media += 1
        if moving and i % 2 == 1:
            cc, off = o["center"], rng.uniform(-0.3, 0.3, 3)
            o["center1"] = {"x": cc["x"] + off[0], "y": cc["y"] + off[1], "z": cc["z"] + off[2]}
    if with_lens and not pinhole:
        cfg["camera"].update(aperture=0.5, focus_dist=7.0)
    sc, c1, lens = _load(host, cfg, width, height, 2, cfg["max_depth"])
    return sc, c1, lens, n_solids, n_media


@pytest.mark.gpu
def test_every_solid_instantiation_is_launched(pkg, abi, host, torch_cuda):
    """(lights, colour map, LDS / L2 tables) x pinhole / lens x static / moving x with / without media x one-shot / accumulating: the 128
    SOLID instantiations, each selected by the scene that should reach it and reporting its key; the accumulated frame is the one-shot's,
    and the grid walk is the full scan's ("variant" 1).  (tests/test_feature_matrix.py compares every one of these cells with the
    restatement.)"""
    torch = torch_cuda
    seen = {}
    for cell in SWEEP_CELLS:
        name, medium = sweep_name(cell), cell[5]
        sc, c1, lens, n_solids, n_media = sweep_world(host, cell, 9, 6)
        gs = _hip_scene(pkg, sc, c1, lens)
        assert gs.query("solids") == n_solids > 1 and (gs.query("media") == n_media) and (n_media > 0) == medium, name
        want = sweep_key(cell)
        one = _one_shot(torch, gs)
        assert gs.query("last_kernel") == want, (name, gs.query("last_kernel"), want)
        seen.setdefault(want, name)
        acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
        segs = 0
        for b, e in ((1, 2), (0, 1)):
            gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
            segs += gs.wait()["segments"]
        assert gs.query("last_kernel") == want | ACCUM, (name, gs.query("last_kernel"))
        seen.setdefault(want | ACCUM, name)
        rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
        gs.resolve(acc.data_ptr(), 2, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
        torch.cuda.current_stream().synchronize()
        _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), f"{name}: accumulated vs one-shot")
        assert segs == one[2]["segments"], name
        gs.set_option("variant", 1)
        full = _one_shot(torch, gs)
        assert gs.query("last_kernel") == want, name
        _same(one, full, f"{name}: grid walk vs full scan")
        assert full[2]["segments"] == one[2]["segments"], name
        gs.close()
    want = SWEEP_KEYS
    assert len(want) == 128 and set(seen) == want, sorted(set(seen) ^ want)


@pytest.mark.gpu
@pytest.mark.parametrize("world", ["unlit", "lit"])
def test_composition_is_the_one_shot_frame(pkg, abi, host, torch_cuda, world):
    """passes (0, 1), (1, 4), (4, 6) through rt_hip_accumulate / rt_hip_resolve, row shards {8, r, 3}, and a second render: each the
    one-shot frame bit for bit"""
    torch = torch_cuda
    cfg = _cfg(_unlit_objs(True) if world == "unlit" else _lit_objs(True), sky=world == "unlit", lens=LENS_KEYS)
    sc, c1, lens = _load(host, cfg, 40, 28, 6, 8, seed=5)
    gs = _hip_scene(pkg, sc, c1, lens)
    one = _one_shot(torch, gs)
    again = _one_shot(torch, gs)
    _same(one, again, "second render")
    assert again[2]["segments"] == one[2]["segments"]
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 4), (4, 6)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") & SOLID and gs.query("last_kernel") & ACCUM
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), 6, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    frame_rgb, frame_lin = np.zeros_like(one[0]), np.zeros_like(one[1])
    segs = 0
    for r in range(3):
        t = abi.RtRowTiles(8, r, 3)
        rows = abi.tiles_global_rows(gs.height, t)
        s_rgb, s_lin, st = _one_shot(torch, gs, t, len(rows))
        frame_rgb[rows], frame_lin[rows] = s_rgb, s_lin
        segs += st["segments"]
    _same(one, (frame_rgb, frame_lin), "row shards")
    assert segs == one[2]["segments"]
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("moving,lens_on", [(False, False), (True, False), (False, True), (True, True)])
def test_first_hit_aovs_and_denoise(pkg, abi, oracle, host, torch_cuda, moving, lens_on):
    """the feature buffers of a solid scene are SolidMini's first hits bit for bit (a solid: the evaluated colour); the denoiser runs"""
    torch = torch_cuda
    sc, c1, lens = _load(host, _cfg(_unlit_objs(moving), lens=LENS_KEYS if lens_on else None), 24, 16, 4, 8, seed=3)
    assert (lens is not None) == lens_on
    gs = _hip_scene(pkg, sc, c1, lens)
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(4, aov.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    want = _mini(oracle, abi, sc, c1, lens).aovs(4)
    got = aov.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    # the ground's two colours both show as albedo: the AOV is the evaluated colour, not the record's `even`
    ground = got[12:, :, 0]
    assert ground.max() > 0.85 and ground.min() < 0.6
    rgb, lin, _ = _one_shot(torch, gs)
    d_lin = torch.from_numpy(lin).to("cuda:0")
    out = torch.zeros_like(d_lin)
    gs.denoise(d_lin.data_ptr(), aov.data_ptr(), d_out_linear=out.data_ptr(), stream=_stream(torch))
    torch.cuda.current_stream().synchronize()
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and not np.array_equal(o, lin)
    frame, _ = gs.refine_to_host_denoised(4)
    assert frame.shape == (16, 24, 3) and frame.any()
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("moving,lens_on", [(False, False), (True, False), (False, True), (True, True)])
def test_first_hit_aovs_with_solids_and_a_medium(pkg, abi, oracle, host, torch_cuda, moving, lens_on):
    """the four rt_aov<LENS, MOTION, true, true> kernels, which no other test launches: the feature buffers of a scene with solids and a
    medium against the first hits of SolidMini — the restatement test_denoise.py compares with (mini_oracle.Mini), which by itself
    knows neither kind of sphere, extended by MediumMini and SolidMini — under test_denoise.py's comparison: bit for bit"""
    from test_denoise import _aovs, _check_aovs
    sc, c1, lens = _load(host, _cfg(_unlit_objs(moving, medium=True), lens=LENS_KEYS if lens_on else None), 24, 16, 2, 8, seed=3)
    gs = _hip_scene(pkg, sc, c1, lens)
    assert gs.query("solids") > 0 and gs.query("media") > 0 and (gs.query("motion") > 0) == moving and gs.query("lens") == lens_on
    got = _aovs(torch_cuda, gs, 2).cpu().numpy()
    gs.close()
    _check_aovs(got, _mini(oracle, abi, sc, c1, lens).aovs(2), "solids and a medium", 2)
    # some pixels' first hits all lie inside the medium (fully covered, zero normal): the frame tells the MEDIUM kernels from the others
    assert ((got[..., 7] == 1.0) & (np.abs(got[..., 4:7]).sum(-1) == 0.0)).any()


WHITE = (C.c_uint8 * 3)(255, 255, 255)      # a 1 x 1 white sky texture: every miss returns 0.7 x (1, 1, 1), whatever its direction


def _ortho_scene(abi, spheres, n, spp, seed, depth=2):
    """the camera of test_medium_gpu._law_scene — at z = 10 looking down -z, vfov 0.1 degrees, 8 x 8 pixels — under a white sky.
    max_depth 2: the camera segment and one bounce.  (With max_depth 1 the ray scattered at the camera segment's hit has depth 0 and is
    black whatever the attenuation, raytracer.rs:71-75: a hit would show nothing of its material.)  A sphere is convex and a diffuse
    bounce leaves along normal + a point inside the unit sphere, so the bounce always reaches the sky: a sample is 0.7 x attenuation."""
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=spp, max_depth=depth, sky_mode=abi.RT_SKY_TEXTURE,
                     spheres=spheres, n_spheres=n, seed=seed)
    sc.sky_rgb8 = C.cast(WHITE, C.POINTER(C.c_uint8))
    sc.sky_w = sc.sky_h = 1
    half = math.tan(math.radians(0.1) / 2.0)
    sc.cam_origin[:] = [0.0, 0.0, 10.0]
    sc.cam_lower_left[:] = [-half, -half, 9.0]
    sc.cam_horizontal[:] = [2.0 * half, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, 2.0 * half, 0.0]
    return sc


@pytest.mark.gpu
def test_the_pattern_rides_a_moving_sphere(pkg, abi, torch_cuda):
    """Independent of the restatement.  A single checker sphere (radius 1 at the origin, even white, odd black, scale 70.5) moves by 1.5
    along the view axis while the camera looks at its centre from z = 10 through a 0.1-degree view.  The camera maps pixel x + jitter to
    u = (x + jitter) / (W - 1), so the view covers -0.00785 < x, y < 0.0101 around the sphere's pole: between -0.56 and 0.72 cells, and the
    frame shows exactly four cells (floor(p_x), floor(p_y) in {-1, 0}; p_z = 70.5 x (1 - at most 1e-4) keeps floor 70), meeting at the
    axis.  As the sphere approaches, a sample's ray meets the sphere's frame at a point scaled TOWARDS the axis — it never leaves its
    quadrant — so every sample keeps its colour: the moving frame is the static frame at the same seed, within the pooled tolerance at
    spp 256.  A world-space pattern sweeps 1.5 x 70.5 = 105 cells of p_z through every pixel over the shutter and turns the frame grey.
    (Along the view axis, as the issue asks: no transverse move is needed for exactness.)"""
    torch = torch_cuda
    frames = []
    for moving in (False, True):
        spheres = (abi.RtSphere * 1)()
        s = spheres[0]
        s.center[:] = [0.0, 0.0, 0.0]
        s.radius = 1.0
        s.kind = abi.RT_MAT_CHECKER
        s.albedo[:] = [1.0, 1.0, 1.0]
        s.tex_w, s.tex_h = abi.checker_odd_pack((0.0, 0.0, 0.0))
        s.h_offset = 70.5
        sc = _ortho_scene(abi, spheres, 1, 256, 99)
        gs = pkg.hip.HipScene(C.pointer(sc), 0, center1=[[0.0, 0.0, 1.5]] if moving else None)
        _, lin, _ = _one_shot(torch, gs)
        k = gs.query("last_kernel")
        assert k & SOLID and bool(k & MOTION) == moving and gs.query("motion") == int(moving)
        frames.append(lin.astype(np.float64))
        gs.close()
    static, moved = frames
    quad = static[:, :, 0]
    # the static frame shows four cells: opposite corners alike, neighbours different, one colour white x 0.7 and the other black
    assert quad[0, 0] == quad[7, 7] and quad[0, 7] == quad[7, 0]
    assert sorted([round(float(quad[0, 0]), 5), round(float(quad[0, 7]), 5)]) == [0.0, 0.7]
    err = float(np.abs(static - moved).max())
    print(f"pattern rides the sphere: max |linear diff| {err:.3g} (tolerance {pooled_atol(256):.3g})")
    assert err <= pooled_atol(256), err


@pytest.mark.gpu
def test_the_mean_of_a_fine_checker_is_the_mean_of_its_colours(pkg, abi, torch_cuda):
    """Independent of the restatement.  The 8 x 8 orthographic-like view (vfov 0.1 degrees from z = 10) looks at the pole of the ground
    sphere (radius 100, centre (0, 0, -100)): a pixel's footprint is about 0.0025 wide, and the scale 20 000 puts about 50 x 50 cells into
    it (>= 64; across the view p_z stays within 0.015 of 2 000 000 from below: one layer, so the parity is that of floor(p_x) + floor(p_y)).
    even = (1, 1, 1), odd = (0, 0, 0), a white sky, max_depth 2 (see _ortho_scene for why not 1): a sample is 0.7 or 0.  The frame's mean
    over the mean of the same scene with a white Lambertian ground is 0.5 within 5 binomial standard deviations of the 8 x 8 x 1024
    samples (0.0098).  The whole view holds about 400 x 400 cells; the partial cells at its rim are at most one row, 1 / 400 of the
    area, so the two colours' shares of the view differ from 1/2 by at most 0.0013 — inside that tolerance."""
    torch = torch_cuda
    spp = 1024
    means = []
    for checker in (True, False):
        spheres = (abi.RtSphere * 1)()
        s = spheres[0]
        s.center[:] = [0.0, 0.0, -100.0]
        s.radius = 100.0
        s.albedo[:] = [1.0, 1.0, 1.0]
        if checker:
            s.kind = abi.RT_MAT_CHECKER
            s.tex_w, s.tex_h = abi.checker_odd_pack((0.0, 0.0, 0.0))
            s.h_offset = 20000.0
        else:
            s.kind = abi.RT_MAT_LAMBERTIAN
        sc = _ortho_scene(abi, spheres, 1, spp, 77)
        gs = pkg.hip.HipScene(C.pointer(sc), 0)
        _, lin, _ = _one_shot(torch, gs)
        assert bool(gs.query("last_kernel") & SOLID) == checker
        means.append(float(lin.astype(np.float64).mean()))
        gs.close()
    n = 8 * 8 * spp
    tol = 5.0 * math.sqrt(0.25 / n)
    ratio = means[0] / means[1]
    print(f"fine checker: mean ratio {ratio:.6f}, expected 0.5, tolerance {tol:.6f}")
    assert abs(means[1] - 0.7) < 1e-5, means[1]
    assert abs(ratio - 0.5) <= tol, (ratio, tol)


@pytest.mark.gpu
def test_solids_with_wide_tables_are_refused_and_bad_records_are_invalid(pkg, abi, host, torch_cuda):
    rng = np.random.default_rng(1)
    cfg = json.loads(FW.big_flat_world_json(66000, rng, 8, 8, 1, 2, half=130.0))
    cfg["objects"][5]["material"] = _chk((0.5, 0.5, 0.5), (0.1, 0.1, 0.1), 2.0)
    sc, _, _ = _load(host, cfg)
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
    for kind, field, v in ((abi.RT_MAT_CHECKER, "h_offset", 0.0), (abi.RT_MAT_NOISE, "h_offset", float("nan")), (abi.RT_MAT_NOISE, "h_offset", float("inf")),
                           (abi.RT_MAT_NOISE, "tex_w", 0), (abi.RT_MAT_NOISE, "tex_w", 17), (abi.RT_MAT_NOISE, "tex_id", 3), (abi.RT_MAT_NOISE, "tex_h", 1 << 32)):
        spheres = (abi.RtSphere * 1)()
        s = spheres[0]
        s.center[:] = [0.0, 0.0, 0.0]
        s.radius, s.kind, s.h_offset, s.tex_w, s.tex_h, s.tex_id = 1.0, kind, 2.0, 7, 0, 0
        s.albedo[:] = [0.5, 0.5, 0.5]
        sc = _ortho_scene(abi, spheres, 1, 1, 1)
        gs = pkg.hip.HipScene(C.pointer(sc), 0)
        assert gs.query("solids") == 1
        gs.close()
        setattr(s, field, v)
        with pytest.raises(pkg.host.RtError) as e:
            pkg.hip.HipScene(C.pointer(sc), 0)
        assert e.value.code == abi.RT_ERR_INVALID, (field, v)


@pytest.mark.gpu
def test_cli_renders_the_example_scene(pkg, host, torch_cuda, tmp_path):
    """the CLI's PNG of scenes/cover_solid_1200x800_spp128.json at a reduced size decodes to the library call's bytes"""
    from PIL import Image
    torch = torch_cuda
    cfg = json.load(open(SOLID_SCENE))
    cfg.update(width=60, height=40, samples_per_pixel=4)
    p = tmp_path / "solid.json"
    p.write_text(json.dumps(cfg))
    sc, c1, ln = _load(host, cfg)
    gs = _hip_scene(pkg, sc, c1, ln)
    want = _one_shot(torch, gs)[0]
    assert gs.query("last_kernel") & SOLID and gs.query("solids") > 3
    gs.close()
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    r = subprocess.run([exe, str(p), str(tmp_path / "solid.png")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "solid.png")), want)
