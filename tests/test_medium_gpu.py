"""Participating media on the GPU, through the C ABI: small frames against the restatement (tests/medium_mini.py),
the grid walk against the full scan on larger worlds, composition with passes / row shards / repeated renders, the first-hit AOVs, and
the transmittance law exp(-2 density) — which is independent of every restatement."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import fuzz_worlds as FW
import medium_mini as MM
from parity import assert_parity, pooled_atol

MEDIUM, MOTION, LENS, ACCUM = 128, 64, 32, 16


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _pt(x, y, z):
    return {"x": float(x), "y": float(y), "z": float(z)}


def _obj(c, r, mat, c1=None):
    o = {"center": _pt(*c), "radius": float(r), "material": mat}
    if c1 is not None:
        o["center1"] = _pt(*c1)
    return o


def _lam(*a):
    return {"Lambertian": {"albedo": list(a)}}


def _med(a, d):
    return {"Medium": {"albedo": list(a), "density": d}}


def _cfg(objs, sky=True, look_from=(0.0, 1.0, 6.0), look_at=(0.0, 0.4, 0.0), vfov=40.0, aspect=1.5, lens=None):
    cam = {"look_from": _pt(*look_from), "look_at": _pt(*look_at), "vup": _pt(0, 1, 0), "vfov": vfov, "aspect": aspect}
    if lens:
        cam.update(lens)
    return {"width": 24, "height": 16, "samples_per_pixel": 4, "max_depth": 8, "sky": {"texture": ""} if sky else None, "camera": cam, "objects": objs}


def _unlit_objs(moving):
    """ground; a medium holding a Lambertian sphere; a glass shell around a second medium; two overlapping media; the enclosing haze
    with the camera inside it.  moving: the media move over the shutter"""
    mv = (lambda c, d: tuple(a + b for a, b in zip(c, d))) if moving else (lambda c, d: None)
    return [
        _obj((0, -100.5, 0), 100.0, _lam(0.5, 0.5, 0.5)),
        _obj((0, 0.5, 0), 1.0, _med((0.9, 0.8, 0.7), 1.2), mv((0, 0.5, 0), (0.3, 0.2, 0.0))),
        _obj((0, 0.5, 0), 0.4, _lam(0.8, 0.2, 0.2)),
        _obj((2.2, 0.3, 0.5), 0.8, {"Glass": {"index_of_refraction": 1.5}}),
        _obj((2.2, 0.3, 0.5), 0.6, _med((0.2, 0.6, 0.9), 3.0), mv((2.2, 0.3, 0.5), (0.0, 0.1, 0.1))),
        _obj((-2.2, 0.3, 0.0), 0.7, _med((0.7, 0.7, 0.2), 2.0), mv((-2.2, 0.3, 0.0), (-0.2, 0.0, 0.3))),
        _obj((-1.7, 0.5, 0.3), 0.6, _med((0.3, 0.9, 0.3), 4.0)),
        _obj((0, 0, 0), 30.0, _med((0.8, 0.8, 0.9), 0.03)),
    ]


def _lit_objs(moving):
    """black sky, one Light, a medium between the light and the ground"""
    mv = (lambda c, d: tuple(a + b for a, b in zip(c, d))) if moving else (lambda c, d: None)
    return [
        _obj((0, -100.5, 0), 100.0, _lam(0.6, 0.6, 0.6)),
        _obj((0, 4.0, 0), 1.0, {"Light": {}}),
        _obj((0, 1.4, 0), 1.0, _med((0.9, 0.9, 0.9), 0.8), mv((0, 1.4, 0), (0.5, 0.0, 0.2))),
        _obj((1.5, 0.0, 1.0), 0.5, _lam(0.2, 0.4, 0.8)),
    ]


def _load(host, cfg, w=None, h=None, spp=None, depth=None, seed=None):
    """(host scene, center1 or None, lens (u, v, r) or None), the lens's focus-plane camera written into RtScene"""
    sc = host.Scene.loads(json.dumps(cfg))
    c = sc.c
    if w:
        c.width, c.height = w, h
    if spp:
        c.samples_per_pixel = spp
    if depth:
        c.max_depth = depth
    if seed is not None:
        c.seed = seed
    lens = None
    cam = cfg["camera"]
    if cam.get("aperture"):
        out = (C.c_double * 2)()
        host.lib().rt_scene_lens(sc._h, out)
        pt = lambda p: (float(p["x"]), float(p["y"]), float(p["z"]))
        d = host.camera_derive_lens(pt(cam["look_from"]), pt(cam["look_at"]), pt(cam["vup"]), float(cam["vfov"]), float(cam["aspect"]), out[0], out[1])
        for i in range(3):
            c.cam_origin[i], c.cam_lower_left[i], c.cam_horizontal[i], c.cam_vertical[i] = (d["origin"][i], d["lower_left_corner"][i],
                                                                                             d["horizontal"][i], d["vertical"][i])
        lens = (d["u"], d["v"], d["lens_radius"])
    return sc, sc.center1(), lens


def _hip_scene(pkg, sc, center1=None, lens=None):
    gs = pkg.hip.HipScene(sc.ptr, 0, center1=center1)
    if lens:
        gs.set_lens(*lens)
    return gs


def _one_shot(torch, gs, tiles=None, rows=None):
    rows = rows if rows is not None else gs.height
    rgb = torch.zeros((rows, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((rows, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.render(rgb.data_ptr(), lin.data_ptr(), tiles, _stream(torch))
    st = gs.wait()
    return rgb.cpu().numpy(), lin.cpu().numpy(), st


def _mini(oracle, abi, sc, center1=None, lens=None):
    L = oracle.lib(abi)
    return MM.MediumMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), center1, lens)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: RGB8 differs at {int((a[0] != b[0]).sum())} values"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: linear radiance differs bitwise"


LENS_KEYS = {"aperture": 0.25, "focus_dist": 6.0}
PARITY_CASES = [(world, variant, depth) for world in ("unlit", "lit") for variant, depth in
                (("plain", 8), ("plain", 50), ("lens", 8), ("moving", 8), ("lens_moving", 8))]


@pytest.mark.gpu
@pytest.mark.parametrize("world,variant,depth", PARITY_CASES)
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, world, variant, depth):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against MediumMini; last_kernel carries MEDIUM"""
    torch = torch_cuda
    moving, lens_on = "moving" in variant, "lens" in variant
    objs = _unlit_objs(moving) if world == "unlit" else _lit_objs(moving)
    cfg = _cfg(objs, sky=world == "unlit", lens=LENS_KEYS if lens_on else None)
    spp = 4 if world == "unlit" else 8
    sc, c1, lens = _load(host, cfg, 24, 16, spp, depth, seed=11 + depth)
    assert (c1 is not None) == moving and (lens is not None) == lens_on
    gs = _hip_scene(pkg, sc, c1, lens)
    assert gs.query("media") == sum("Medium" in o["material"] for o in objs)
    rgb, lin, st = _one_shot(torch, gs)
    k = gs.query("last_kernel")
    assert k & MEDIUM and bool(k & MOTION) == moving and bool(k & LENS) == lens_on and bool(k & 4) == (world == "lit"), k
    m = _mini(oracle, abi, sc, c1, lens)
    m_rgb, m_lin, m_segs = m.render()
    print(f"{world} {variant} depth {depth}: max |linear diff| {float(np.abs(lin - m_lin).max()):.3g}, segments gpu {st['segments']} mini {m_segs} - {m.discarded}")
    assert_parity(rgb, lin, m_rgb, m_lin, f"{world} {variant}", atol=pooled_atol(spp))
    assert st["segments"] == m_segs - m.discarded, (st["segments"], m_segs, m.discarded)
    if world == "unlit":
        assert m.discarded == 0
    # ... and the full scan ("variant" 1), the second device-side answer, gives the same frame bit for bit
    gs.set_option("variant", 1)
    b = _one_shot(torch, gs)
    _same((rgb, lin), b, "variant 1")
    assert b[2]["segments"] == st["segments"]
    gs.close()


def _with_media(cfg_text, rng, quarter=4):
    """a fuzz world with a seeded quarter of its non-light spheres (positive radius) turned into media"""
    cfg = json.loads(cfg_text)
    n = 0
    for o in cfg["objects"]:
        if "Light" in o["material"] or o["radius"] <= 0 or o["radius"] > 100:
            continue
        if rng.integers(quarter) == 0:
            o["material"] = _med([round(float(v), 3) for v in rng.uniform(0.2, 1.0, 3)], round(float(10.0 ** rng.uniform(-1.0, 1.0)) / o["radius"], 4))
            n += 1
    return cfg, n


TRIANGLE = {"cluster": lambda rng: FW.fuzz_world_json(rng, 0, 48, 32, 2, 8), "decades": lambda rng: FW.fuzz_world_json(rng, 1, 48, 32, 2, 8),
            "in_glass": lambda rng: FW.fuzz_world_json(rng, 2, 48, 32, 2, 8), "layer": lambda rng: FW.fuzz_world_json(rng, 3, 48, 32, 2, 8),
            "far": lambda rng: FW.fuzz_world_json(rng, 4, 48, 32, 2, 8), "sparse": lambda rng: FW.fuzz_world_json(rng, 5, 48, 32, 2, 8),
            "l2_6001": lambda rng: FW.big_flat_world_json(6000, rng, 48, 32, 2, 6, half=40.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TRIANGLE))
def test_grid_walk_equals_full_scan_on_larger_worlds(pkg, host, torch_cuda, name):
    """tests/fuzz_worlds.py kinds with a quarter of the spheres turned into media: grid walk = "variant" 1, bit for bit, equal path counts"""
    torch = torch_cuda
    rng = np.random.default_rng(4200 + sorted(TRIANGLE).index(name))
    cfg, n_media = _with_media(TRIANGLE[name](rng), rng)
    assert n_media >= 10
    sc, _, _ = _load(host, cfg)
    gs = _hip_scene(pkg, sc)
    assert gs.query("media") == n_media and gs.query("grid_cells") > 0
    a = _one_shot(torch, gs)
    assert gs.query("last_kernel") & MEDIUM
    if name == "l2_6001":
        assert gs.query("lds_tables") == 0, "6 001 spheres: the tables sit in L2"
    gs.set_option("variant", 1)
    b = _one_shot(torch, gs)
    _same(a, b, name)
    assert a[2]["segments"] == b[2]["segments"] and a[2]["segments"] > 48 * 32 * 2
    assert b[2]["exact_tests"] > a[2]["exact_tests"]
    gs.close()


@pytest.mark.gpu
def test_one_gridded_world_against_the_restatement(pkg, abi, oracle, host, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(4300)
    cfg, n_media = _with_media(FW.fuzz_world_json(rng, 2, 16, 12, 2, 8), rng)
    sc, _, _ = _load(host, cfg)
    gs = _hip_scene(pkg, sc)
    assert gs.query("grid_cells") > 0 and n_media > 10
    rgb, lin, st = _one_shot(torch, gs)
    m = _mini(oracle, abi, sc)
    m_rgb, m_lin, m_segs = m.render()
    assert_parity(rgb, lin, m_rgb, m_lin, "gridded world", atol=pooled_atol(2))
    assert st["segments"] == m_segs - m.discarded
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", ["unlit", "lit"])
def test_composition_is_the_one_shot_frame(pkg, abi, host, torch_cuda, world):
    """passes through rt_hip_accumulate / rt_hip_resolve, row shards of 8 (the ranks of a 3-rank group), and a second render (the
    learnt queue order): each the one-shot frame bit for bit"""
    torch = torch_cuda
    cfg = _cfg(_unlit_objs(True) if world == "unlit" else _lit_objs(True), sky=world == "unlit", lens=LENS_KEYS)
    sc, c1, lens = _load(host, cfg, 40, 28, 6, 8, seed=5)
    gs = _hip_scene(pkg, sc, c1, lens)
    one = _one_shot(torch, gs)
    again = _one_shot(torch, gs)
    _same(one, again, "second render")
    assert again[2]["segments"] == one[2]["segments"]
    # passes
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 4), (4, 6)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") & MEDIUM and gs.query("last_kernel") & ACCUM
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), 6, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    # row shards of 8 over 3 ranks
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
    """the feature buffers of a medium scene are MediumMini's first hits (a medium: its albedo, normal 0, 1 / t); the denoiser runs"""
    torch = torch_cuda
    sc, c1, lens = _load(host, _cfg(_unlit_objs(moving), lens=LENS_KEYS if lens_on else None), 24, 16, 4, 8, seed=3)
    assert (lens is not None) == lens_on     # (the four MEDIUM rt_aov kernels without SOLID: pinhole / lens x static / moving)
    gs = _hip_scene(pkg, sc, c1, lens)
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(4, aov.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    want = _mini(oracle, abi, sc, c1, lens).aovs(4)
    got = aov.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    # some pixels' first hits all lie inside a medium: fully covered, with a zero normal
    assert ((got[..., 7] == 1.0) & (np.abs(got[..., 4:7]).sum(-1) == 0.0)).any()
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


def _law_scene(abi, media, moving):
    """a camera at z = 10 looking down -z at media of radius 1 around the origin, vfov 0.1 degrees, 8 x 8 pixels, 4096 samples, the
    gradient sky; the camera's vectors scaled by 3 so that ray directions have length 3"""
    n = max(1, len(media))
    spheres = (abi.RtSphere * n)()
    for i, d in enumerate(media):
        spheres[i].center[:] = [0.0, 0.0, 0.0]
        spheres[i].radius = 1.0
        spheres[i].kind = abi.RT_MAT_MEDIUM
        spheres[i].fuzz_or_ior = d
        spheres[i].albedo[:] = [0.0, 0.0, 0.0]
    if not media:   # the same frame without the medium: one small Lambertian sphere behind the camera
        spheres[0].center[:] = [0.0, 0.0, 50.0]
        spheres[0].radius = 0.5
        spheres[0].kind = abi.RT_MAT_LAMBERTIAN
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=4096, max_depth=8, sky_mode=1, spheres=spheres, n_spheres=n, seed=77)
    half = 3.0 * math.tan(math.radians(0.1) / 2.0)
    sc.cam_origin[:] = [0.0, 0.0, 10.0]
    sc.cam_lower_left[:] = [-half, -half, 10.0 - 3.0]
    sc.cam_horizontal[:] = [2.0 * half, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, 2.0 * half, 0.0]
    c1 = [[0.0, 0.0, 1.5]] * n if moving else None
    return sc, spheres, c1


LAW_CASES = {"thin": ([0.4], False), "dense": ([1.3], False), "concentric": ([0.3, 0.45], False), "moving_along_the_view": ([0.7], True)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LAW_CASES))
def test_transmittance_law(pkg, abi, torch_cuda, case):
    """mean radiance through an absorbing medium (albedo 0) of radius 1 / the same frame's mean without it = exp(-2 sum of densities),
    within 5 binomial standard deviations of 262 144 samples.  Two concentric media must multiply: that fails if they share a draw."""
    torch = torch_cuda
    media, moving = LAW_CASES[case]
    means = []
    for m in (media, []):
        sc, keep, c1 = _law_scene(abi, m, moving and bool(m))
        gs = pkg.hip.HipScene(C.pointer(sc), 0, center1=c1)
        _, lin, st = _one_shot(torch, gs)
        assert bool(gs.query("last_kernel") & MEDIUM) == bool(m)
        means.append(float(lin.astype(np.float64).mean()))
        gs.close()
    p = math.exp(-2.0 * sum(media))
    tol = 5.0 * math.sqrt(p * (1.0 - p) / 262144.0)
    ratio = means[0] / means[1]
    print(f"{case}: transmitted {ratio:.6f}, law {p:.6f}, tolerance {tol:.6f}")
    assert abs(ratio - p) <= tol, (case, ratio, p, tol)


@pytest.mark.gpu
def test_media_with_wide_tables_are_refused(pkg, abi, host, torch_cuda):
    rng = np.random.default_rng(1)
    cfg = json.loads(FW.big_flat_world_json(66000, rng, 8, 8, 1, 2, half=130.0))
    cfg["objects"][5]["material"] = _med((0.5, 0.5, 0.5), 1.0)
    sc, _, _ = _load(host, cfg)
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
