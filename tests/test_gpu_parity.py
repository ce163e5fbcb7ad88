"""Parity tests proper: the HIP megakernel, called through the C ABI (librt_hip.so), against
the CPU oracle on identical Philox seeds, against the committed golden fixtures, and — at
BASELINE.json's full size — through size-independent properties.  Needs a real MI355X."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from fuzz_worlds import adversarial_scene, fuzz_world_json
from conftest import dvec
from parity import assert_parity, pooled_atol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "scenes"))

CASES = {
    "cover_96x64_spp4": ("cover", 96, 64, 4, 50, 0),
    "cover_60x40_spp2_seed7": ("cover", 60, 40, 2, 50, 7),
    "test_80x60_spp4": ("test", 80, 60, 4, 8, 0),
    "test_40x30_spp8_depth50": ("test", 40, 30, 8, 50, 3),
    "cover_tex_64x36_spp4": ("cover4k_tex", 64, 36, 4, 50, 0),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def gpu_render(pkg, abi, torch_cuda):
    torch = torch_cuda

    def _render(scene, tiles=None, variant=0, want_linear=True, chunk_spp=None, tile_log2=None, tile_order=None, frames=1, tile_shape=None,
                tile_affinity=None, opts=None, library=None, query=None):
        """variant 0: the product kernel (grid walk, tile queue, exact fixed-point pixel sums);
        variant 1: same kernel, the reference's brute force over all spheres.  chunk_spp: samples of a
        pixel per work item; tile_log2: pixel tiles of 2^k x 2^k."""
        sc = scene.c
        rows = abi.tiles_local_rows(sc.height, tiles)
        gs = pkg.hip.HipScene(scene.ptr, 0, library=library)   # (library: probe_lib() for the tests that force the wide table format)
        if query is not None:
            query.update({k: gs.query(k) for k in ("grid_wide", "grid_cells", "grid_items", "grid_large")})
        if variant:
            gs.set_option("variant", variant)
        if chunk_spp is not None:
            gs.set_option("chunk_spp", chunk_spp)
        if tile_log2 is not None:
            gs.set_option("tile_log2", tile_log2)
        if tile_order is not None:
            gs.set_option("tile_order", tile_order)
        if tile_shape is not None:
            gs.set_option("tile_shape", tile_shape)
        if tile_affinity is not None:
            gs.set_option("tile_affinity", tile_affinity)
        for k, v in (opts or {}).items():
            gs.set_option(k, v)
        rgb = torch.zeros((rows, sc.width, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((rows, sc.width, 3), dtype=torch.float32, device="cuda:0") if want_linear else None
        for _ in range(frames):   # (frames > 1: the later frames use the queue order learnt from the one before)
            gs.render(rgb.data_ptr(), lin.data_ptr() if want_linear else 0, tiles, torch.cuda.current_stream().cuda_stream)
            st = gs.wait()
        out = rgb.cpu().numpy(), (lin.cpu().numpy() if want_linear else None), st
        gs.close()
        return out
    return _render


def test_gpu_math_is_ieee_exact(pkg, oracle, abi, torch_cuda):
    """bit-parity with the CPU oracle needs correctly rounded f64 sqrt/div and f32 sqrt on
    the GPU, and the shared atan2 (csrc/common/rt_atan2.h, texture u) to give the oracle's bits."""
    torch = torch_cuda
    n = 1 << 20
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.random(n // 2), 10.0 ** rng.uniform(-30, 30, n // 2)])
    # the library's square root rescales arguments below 2^-767: both sides of that threshold, denormals, the
    # largest finite values, perfect squares and their neighbours, 0 and inf
    k = 4096
    sq = rng.integers(1, 1 << 26, k).astype(np.float64) ** 2
    x[:12 * k] = np.concatenate([2.0 ** rng.uniform(-780, -755, k), 2.0 ** rng.uniform(-1074, -1000, k), 2.0 ** rng.uniform(1000, 1023.99, k),
                                 2.0 ** rng.uniform(-1022, 1023, 4 * k), sq, np.nextafter(sq, 0), np.nextafter(sq, np.inf),
                                 np.array([0.0, 2.0 ** -767, np.nextafter(2.0 ** -767, 0), np.finfo(np.float64).max, np.inf, 5e-324] * (k // 6) + [0.0] * (k % 6)),
                                 rng.random(k) * 1e-300])
    y = np.concatenate([rng.random(n // 2) + 1e-3, 10.0 ** rng.uniform(-30, 30, n // 2)])
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    o_sqrt, o_div, o_at = torch.empty_like(dx), torch.empty_like(dx), torch.empty_like(dx)
    o_sqrtf = torch.empty(n, dtype=torch.float32, device="cuda")
    rc = pkg.hip.probe_lib().rt_hip_math_probe(dx.data_ptr(), dy.data_ptr(), o_sqrt.data_ptr(), o_div.data_ptr(), o_sqrtf.data_ptr(),
                                         o_at.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(o_sqrt.cpu().numpy(), np.sqrt(x))
    with np.errstate(all="ignore"):
        assert np.array_equal(o_div.cpu().numpy(), x / y, equal_nan=True)
    with np.errstate(all="ignore"):
        assert np.array_equal(o_sqrtf.cpu().numpy(), np.sqrt(x.astype(np.float32)))
    fin = np.flatnonzero(np.isfinite(x))[: 1 << 18]
    at = o_at.cpu().numpy()[fin]
    f = oracle.lib(abi).rt_oracle_atan2
    want = np.array([f(a, b) for a, b in zip((x[fin] - 0.5).tolist(), (y[fin] - 0.5).tolist())])
    assert np.array_equal(at, want), np.flatnonzero(at != want)[:10]          # device build == CPU build of the one routine
    assert np.allclose(at, np.arctan2(x[fin] - 0.5, y[fin] - 0.5), rtol=3e-16, atol=0)   # and it is atan2 (1 ulp of numpy's)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_oracle_and_golden(name, gpu_render, oracle, hostsim, abi, load_scene):
    scene, w, h, spp, depth, seed = CASES[name]
    sc = load_scene(scene, w, h, spp, depth, seed)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    # the oracle is all-IEEE (atan2 included): the frozen files are its bits on this box too
    assert np.array_equal(o_rgb, g["rgb8"]) and np.array_equal(o_lin, g["linear"]) and o_st["segments"] == int(g["segments"])
    # the product kernel: same paths (grid walk = the reference's closest hit, same texels), exact fixed-point pixel sums
    p_rgb, p_lin, p_st = gpu_render(sc)
    p_err, p_flips = assert_parity(p_rgb, p_lin, o_rgb, o_lin, name + " product vs oracle", atol=pooled_atol(spp), flip_frac=5e-4)
    assert_parity(p_rgb, p_lin, g["rgb8"], g["linear"], name + " product vs golden", atol=pooled_atol(spp), flip_frac=5e-4)
    # CPU build of the same per-lane code with fixed-point sums: integer sums are order-free -> bit-exact, textures included
    h_rgb, h_lin, h_st = hostsim.render(sc.ptr, None, 3 + 16)
    assert np.array_equal(p_lin, h_lin) and np.array_equal(p_rgb, h_rgb)
    assert p_st["exact_tests"] == h_st["exact_tests"] and p_st["grid_steps"] == h_st["grid_steps"]
    for cs, tl in ((1, 3), (3, 2), (spp, 1), (2, 0), (spp, 3)):  # chunking and pixel-tile size change no bit
        c_rgb, c_lin, c_st = gpu_render(sc, chunk_spp=cs, tile_log2=tl)
        assert np.array_equal(c_rgb, p_rgb) and np.array_equal(c_lin, p_lin) and c_st["segments"] == p_st["segments"], (cs, tl)
    assert p_st["samples"] == w * h * spp == o_st["samples"]
    # the kernel traces every segment the reference traces, minus the light loops whose sum raytracer.rs:124 discards
    assert p_st["segments"] == o_st["segments"] - o_st["segments_discarded"] == int(g["segments"]) - int(g["segments_discarded"])
    assert (o_st["segments_discarded"] > 0) == bool(sc.lights())
    assert p_st["sphere_tests"] == p_st["segments"] * sc.c.n_spheres and p_st["tex_oob"] == 0
    print(f"{name}: max|dlin|={p_err:.2e} rgb8 flips={p_flips} "
          f"exact/segment={p_st['exact_tests'] / max(1, p_st['segments']):.2f} steps/segment={p_st['grid_steps'] / max(1, p_st['segments']):.2f}")


@pytest.mark.parametrize("scene,w,h,spp,depth", [("cover", 64, 48, 3, 50), ("test", 48, 36, 3, 8)])
def test_grid_variant_equals_bruteforce_variant(gpu_render, load_scene, scene, w, h, spp, depth):
    """variant 1 runs the reference's exact test on every sphere (no grid): same bits as the grid walk."""
    sc = load_scene(scene, w, h, spp, depth)
    a_rgb, a_lin, a_st = gpu_render(sc, variant=0)
    b_rgb, b_lin, b_st = gpu_render(sc, variant=1)
    assert np.array_equal(a_rgb, b_rgb) and np.array_equal(a_lin, b_lin)
    assert a_st["segments"] == b_st["segments"]
    assert b_st["exact_tests"] == b_st["sphere_tests"] >= a_st["exact_tests"] and b_st["grid_steps"] == 0
    if sc.c.n_spheres > 64:
        assert a_st["grid_steps"] > 0 and a_st["exact_tests"] < 0.05 * a_st["sphere_tests"]


def test_work_distribution_stress(gpu_render, load_scene):
    """The tile-slot protocol under contention: thousands of one-pixel tiles with one-sample chunks
    (every acquire opens or re-opens a slot), big tiles with tiny chunks, ragged image edges — the
    frame and the path count never change, run after run."""
    sc = load_scene("cover", 203, 117, 5, 50)  # neither dimension a multiple of any tile size
    ref_rgb, ref_lin, ref_st = gpu_render(sc)
    for shape in (0, 1, 2, 3):   # tiles as squares (8x8 ... 1x1, the default), scanline runs (64x1 ... 1x1), 16x4, 32x2
        for tl, cs in ((0, 1), (0, 5), (1, 1), (2, 2), (3, 1), (3, 5), (1, 3)) if shape < 2 else ((1, 1), (2, 2), (3, 1), (3, 5)):
            for _ in range(2):
                rgb, lin, st = gpu_render(sc, chunk_spp=cs, tile_log2=tl, tile_shape=shape)
                assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin), (shape, tl, cs)
                assert st["segments"] == ref_st["segments"] and st["samples"] == 203 * 117 * 5
    # per-XCD queues forced on for this small, ragged frame (tile_affinity = 2): partial last run, one-pixel tiles, every
    # queue order, stealing from the first tile on — same frame
    for tl, cs, order in ((0, 1, 2), (0, 5, 1), (1, 1, 0), (2, 2, 2), (3, 1, 2), (3, 5, 0)):
        rgb, lin, st = gpu_render(sc, chunk_spp=cs, tile_log2=tl, tile_order=order, tile_affinity=2, frames=3 if order == 2 else 1)
        assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin) and st["segments"] == ref_st["segments"], ("affinity", tl, cs, order)
    # tiles taken from the queue 1 / 3 / 64 at a time (the workgroup's stash): one queue and per-XCD queues, every order, and
    # batches larger than a queue's share (the taper, the clipped last batch, a frame with fewer tiles than one batch)
    for batch in (1, 3, 64):
        for tl, cs, order, aff in ((0, 1, 2, 0), (0, 5, 1, 2), (1, 1, 0, 2), (2, 2, 2, 2), (3, 1, 2, 0), (3, 5, 0, 2)):
            rgb, lin, st = gpu_render(sc, chunk_spp=cs, tile_log2=tl, tile_order=order, tile_affinity=aff, frames=3 if order == 2 else 1,
                                      opts={"tile_batch": batch})
            assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin) and st["segments"] == ref_st["segments"], ("batch", batch, tl, cs, order, aff)
    # the lit kernel (parked light frames in LDS beside the tile slots) under the same contention
    lit = load_scene("test", 101, 67, 6, 8)
    l_rgb, l_lin, l_st = gpu_render(lit)
    for shape, tl, cs in ((0, 0, 1), (0, 1, 2), (0, 3, 1), (1, 2, 3), (2, 3, 6), (3, 3, 2)):
        rgb, lin, st = gpu_render(lit, chunk_spp=cs, tile_log2=tl, tile_shape=shape)
        assert np.array_equal(rgb, l_rgb) and np.array_equal(lin, l_lin), ("lit", shape, tl, cs)
        assert st["segments"] == l_st["segments"]
    # a frame whose width is a multiple of 4 takes the dword-packed framebuffer stores (tiles >= 4 pixels wide), others bytes
    for w in (204, 202):
        sc2 = load_scene("cover", w, 31, 3, 50)
        a_rgb, a_lin, _ = gpu_render(sc2, tile_log2=0)          # 1-pixel tiles: always byte stores
        for shape, tl in ((1, 1), (1, 2), (1, 3), (0, 2), (0, 3), (2, 3), (3, 3), (2, 1)):
            b_rgb, b_lin, _ = gpu_render(sc2, tile_log2=tl, tile_shape=shape)
            assert np.array_equal(a_rgb, b_rgb) and np.array_equal(a_lin, b_lin), (w, shape, tl)
    # the order in which tiles leave the queue (top row first / bottom row first / deepest tiles of the previous frame
    # first, over three frames of one resident scene) changes nothing either
    for order in (0, 1, 2):
        for tl in (None, 0, 3):
            rgb, lin, st = gpu_render(sc, tile_order=order, tile_log2=tl, frames=3 if order == 2 else 1)
            assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin), (order, tl)
            assert st["segments"] == ref_st["segments"]


@pytest.mark.parametrize("world", [2, 3, 8])
def test_row_tile_shards_reassemble_bit_identically(gpu_render, abi, load_scene, world):
    sc = load_scene("cover", 72, 45, 3, 50)
    full_rgb, full_lin, _ = gpu_render(sc)
    seen = 0
    for rank in range(world):
        t = abi.RtRowTiles(2 if world == 8 else 8, rank, world)
        rows = abi.tiles_global_rows(45, t)
        rgb, lin, st = gpu_render(sc, tiles=t)
        assert np.array_equal(rgb, full_rgb[rows]) and np.array_equal(lin, full_lin[rows])
        assert st["samples"] == len(rows) * 72 * 3
        seen += len(rows)
    assert seen == 45


def test_degenerate_scenes(gpu_render, oracle, abi, host):
    base = ('{"width":9,"height":5,"samples_per_pixel":3,"max_depth":%d,"sky":%s,"camera":{"look_from":{"x":0.0,"y":0.0,"z":0.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":-1.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":90.0,"aspect":1.8},"objects":[%s]}')
    lam = '{"center":{"x":0.0,"y":0.0,"z":-1.0},"radius":0.5,"material":{"Lambertian":{"albedo":[0.8,0.3,0.3]}}}'
    light = '{"center":{"x":0.0,"y":3.0,"z":-1.0},"radius":1.0,"material":{"Light":{}}}'
    bright = '{"center":{"x":0.0,"y":-100.5,"z":-1.0},"radius":100.0,"material":{"Metal":{"albedo":[1.5,0.2,2.0],"fuzz":0.3}}}'
    for depth in (0, 1, 2, 5):
        for sky in ("null", '{"texture":""}'):
            for objs in ("", lam, lam + "," + light, light + "," + lam + "," + light + "," + bright):
                sc = host.Scene.loads(base % (depth, sky, objs))
                o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
                for variant in (0, 1):
                    rgb, lin, st = gpu_render(sc, variant=variant)
                    assert_parity(rgb, lin, o_rgb, o_lin, f"depth {depth} sky {sky} objs {len(objs)} variant {variant}", atol=pooled_atol(3))
                    assert st["segments"] == o_st["segments"] - o_st["segments_discarded"]


@pytest.mark.parametrize("w,h", [(1, 1), (1, 4), (5, 1)])
def test_one_pixel_wide_or_high_frames(gpu_render, oracle, hostsim, abi, host, w, h):
    """width - 1 = 0 or height - 1 = 0: the reference divides by zero (raytracer.rs:199-200), every ray is NaN/inf and
    every sample NaN.  The kernel's fixed-point pixel sums cannot hold a NaN: the sample adds 0 and flags the pixel in
    the tile's NaN mask, so the linear image reads NaN exactly where the oracle's f32 sum does, and the RGB8 byte is
    what f32 -> u8 makes of NaN on both sides (255 under our restatement of palette — unpinned)."""
    text = ('{"width":%d,"height":%d,"samples_per_pixel":3,"max_depth":5,"sky":{"texture":""},"camera":{"look_from":{"x":0.0,"y":0.0,"z":0.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":-1.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":90.0,"aspect":1.8},"objects":['
            '{"center":{"x":0.0,"y":0.0,"z":-1.0},"radius":0.5,"material":{"Lambertian":{"albedo":[0.8,0.3,0.3]}}}]}' % (w, h))
    sc = host.Scene.loads(text)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    assert np.isnan(o_lin).all() and (o_rgb == 255).all()
    h_rgb, h_lin, _ = hostsim.render(sc.ptr, None, 3 + 16)
    assert np.array_equal(h_rgb, o_rgb) and np.isnan(h_lin).all()
    for variant in (0, 1):
        for tl in (None, 0, 3):
            rgb, lin, st = gpu_render(sc, variant=variant, tile_log2=tl)
            assert np.array_equal(rgb, o_rgb), (variant, rgb.ravel())
            assert np.isnan(lin).all()
            assert st["segments"] == o_st["segments"] == w * h * 3


def test_nan_samples_flag_only_their_pixel_and_channel(gpu_render, oracle, abi, host):
    """a NaN albedo channel poisons exactly the pixels / channels whose paths touch that sphere (the reference's f32
    sum goes NaN there, raytracer.rs:203-205); every other value keeps its bits"""
    text = ('{"width":48,"height":32,"samples_per_pixel":4,"max_depth":6,"sky":{"texture":""},"camera":{"look_from":{"x":0.0,"y":0.5,"z":1.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":-1.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":70.0,"aspect":1.5},"objects":['
            '{"center":{"x":0.0,"y":-100.5,"z":-1.0},"radius":100.0,"material":{"Lambertian":{"albedo":[0.6,0.6,0.6]}}},'
            '{"center":{"x":-0.6,"y":0.0,"z":-1.0},"radius":0.5,"material":{"Lambertian":{"albedo":[0.8,0.3,0.3]}}},'
            '{"center":{"x":0.6,"y":0.0,"z":-1.0},"radius":0.5,"material":{"Metal":{"albedo":[0.8,0.8,0.8],"fuzz":0.1}}}]}')
    sc = host.Scene.loads(text)
    sc.c.spheres[1].albedo[1] = float("nan")          # green channel of the left sphere
    o_rgb, o_lin, _ = oracle.render(abi, sc.ptr)
    nan = np.isnan(o_lin)
    assert nan[..., 1].any() and not nan[..., 0].any() and not nan[..., 2].any() and not nan[..., 1].all()
    for tl in (None, 0, 2, 3):
        rgb, lin, _ = gpu_render(sc, tile_log2=tl)
        assert np.array_equal(np.isnan(lin), nan), tl
        assert np.array_equal(rgb, o_rgb) or np.abs(rgb.astype(int) - o_rgb.astype(int)).max() <= 1
        assert np.abs(np.where(nan, 0.0, lin) - np.where(nan, 0.0, o_lin)).max() <= pooled_atol(4)
        assert (rgb[nan] == 255).all()


def test_many_lights_nested_sampling(gpu_render, oracle, abi, host):
    """several lights + occluders: exercises the nested light-ray stack (raytracer.rs:103-110)"""
    objs = ['{"center":{"x":0.0,"y":-100.5,"z":-1.0},"radius":100.0,"material":{"Lambertian":{"albedo":[0.7,0.7,0.7]}}}']
    for i, x in enumerate((-2.0, 0.0, 2.0)):
        objs.append('{"center":{"x":%f,"y":2.5,"z":-2.0},"radius":0.5,"material":{"Light":{}}}' % x)
        objs.append('{"center":{"x":%f,"y":0.0,"z":-1.5},"radius":0.5,"material":{"%s}}' %
                    (x, ['Lambertian":{"albedo":[0.9,0.2,0.2]}', 'Glass":{"index_of_refraction":1.5}', 'Metal":{"albedo":[0.8,0.8,0.9],"fuzz":0.2}'][i]))
        objs.append('{"center":{"x":%f,"y":1.2,"z":-1.8},"radius":0.3,"material":{"Lambertian":{"albedo":[0.3,0.9,0.4]}}}' % x)
    text = ('{"width":64,"height":40,"samples_per_pixel":16,"max_depth":6,"sky":null,"camera":{"look_from":{"x":0.0,"y":1.0,"z":3.0},'
            '"look_at":{"x":0.0,"y":0.5,"z":-1.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":60.0,"aspect":1.6},"objects":[' + ",".join(objs) + "]}")
    sc = host.Scene.loads(text)
    assert len(sc.lights()) == 3
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    for variant in (0, 1):
        rgb, lin, st = gpu_render(sc, variant=variant)
        assert_parity(rgb, lin, o_rgb, o_lin, f"3 lights variant {variant}", atol=pooled_atol(16))
        assert o_lin.max() > 0.05 and st["segments"] > st["samples"]
        assert o_st["segments_discarded"] > 0 and st["segments"] == o_st["segments"] - o_st["segments_discarded"]


def test_light_draw_words_and_the_open_high_word(gpu_render, oracle, abi, host):
    """A lit kernel decides the light-sampling draw (raytracer.rs:100) of a hit that is not Glass from its HIGH word — the word
    attempt 0's Philox call leaves over — and calls for the low word only when that leaves `draw > threshold` open: one high word
    in 2^32.  tests/light_draw_cases.py holds seeds (found offline) that put pixel 0's first hit there, with the low word deciding
    either way: the kernel must trace the oracle's paths — a decision taken from the high word alone misses or adds the light
    ray of pixel 0, and the segment identity fails.  Also at a size where other lanes of the wave take the ordinary route."""
    import light_draw_cases as ldc
    for seed, samples in ldc.OPEN_SEEDS.items():
        for w, h, spp in ((2, 2, 1), (40, 24, 4)):
            sc = host.Scene.loads(ldc.scene_json(width=w, height=h, spp=spp))
            sc.c.seed = seed
            o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
            rgb, lin, st = gpu_render(sc)
            assert_parity(rgb, lin, o_rgb, o_lin, f"seed {seed} {w}x{h}", atol=pooled_atol(spp))
            assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (seed, samples, w, h)


def test_lit_cover_scene_light_frame_pool(gpu_render, oracle, abi, host):
    """A lit scene of cover size: 1024 per-lane light frames (80 KB) would push the tables out of LDS, so the workgroup
    shares a POOL of frames (rt_core.h LightState<true, true>; one light: 160 records for ~66 in use).  A lane that
    finds the pool exhausted repeats its segment.  The frame must not depend on any of it: the automatic pool, a pool of
    32 records (most light-sampling hits repeat, some many times) and — two lights, forced — pools of 64 and 32 all give
    the oracle's image and exactly the oracle's path count (a repeated segment is counted once)."""
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")))
    cfg.update(width=240, height=160, samples_per_pixel=16)
    cfg["objects"].append({"center": {"x": 0.0, "y": 30.0, "z": 10.0}, "radius": 8.0, "material": {"Light": {}}})
    one = host.Scene.loads(json.dumps(cfg))
    cfg["objects"].append({"center": {"x": 3.0, "y": 2.5, "z": 2.0}, "radius": 0.4, "material": {"Light": {}}})
    two = host.Scene.loads(json.dumps(cfg))
    cfg["objects"].pop()
    cfg["objects"][5]["material"] = {"Lambertian": {"albedo": [1.5, 0.9, 0.2]}}   # an albedo above 1: the GENERAL colour map beside the pool
    hot = host.Scene.loads(json.dumps(cfg))
    for sc, pools in ((one, (0, 32, 96)), (two, (0, 64, 32)), (hot, (0, 64))):
        o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
        first = None
        for pool in pools:
            rgb, lin, st = gpu_render(sc, opts={"light_pool": pool})
            assert_parity(rgb, lin, o_rgb, o_lin, f"lit cover, {len(sc.lights())} light(s), pool {pool}", atol=pooled_atol(16))
            assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (pool, st["segments"])
            first = first if first is not None else (rgb, lin)
            assert np.array_equal(rgb, first[0]) and np.array_equal(lin, first[1]), pool   # and bit-identical to one another
            print(f"lit cover {len(sc.lights())} light(s) pool {pool}: kernel {st['kernel_ms']:.3f} ms")


def test_light_pools_repeats_and_the_hbm_overflow(pkg, gpu_render, oracle, abi, host, torch_cuda, load_scene):
    """The light records of a lit kernel live in two LDS pools of the workgroup (frames, colour-map bases; rt_core.h) — no
    per-lane scratch object.  Three lights and occluders: a third of the light rays' own hits start sampling the lights
    again (nested activations, linked pool records).  The frame must not depend on where a record came from: tiny frame
    pool (camera-path hits repeat their segment, nested ones overflow to HBM), tiny base pool (repeats), nested
    activations ALWAYS through the HBM overflow, and all of it at once give the automatic pools' frame bit for bit, the
    oracle's image and exactly the oracle's path count."""
    objs = ['{"center":{"x":0.0,"y":-100.5,"z":-1.0},"radius":100.0,"material":{"Lambertian":{"albedo":[0.7,0.7,0.7]}}}']
    for i, x in enumerate((-2.0, 0.0, 2.0)):
        objs.append('{"center":{"x":%f,"y":2.5,"z":-2.0},"radius":0.5,"material":{"Light":{}}}' % x)
        objs.append('{"center":{"x":%f,"y":0.0,"z":-1.5},"radius":0.5,"material":{"%s}}' %
                    (x, ['Lambertian":{"albedo":[0.9,0.2,0.2]}', 'Glass":{"index_of_refraction":1.5}', 'Metal":{"albedo":[0.8,0.8,0.9],"fuzz":0.2}'][i]))
        objs.append('{"center":{"x":%f,"y":1.2,"z":-1.8},"radius":0.3,"material":{"Lambertian":{"albedo":[0.3,0.9,0.4]}}}' % x)
    text = ('{"width":200,"height":120,"samples_per_pixel":16,"max_depth":6,"sky":null,"camera":{"look_from":{"x":0.0,"y":1.0,"z":3.0},'
            '"look_at":{"x":0.0,"y":0.5,"z":-1.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":60.0,"aspect":1.6},"objects":[' + ",".join(objs) + "]}")
    for general_map in (False, True):
        sc = host.Scene.loads(text.replace("[0.9,0.2,0.2]", "[1.4,0.2,0.2]") if general_map else text)   # an albedo above 1: the general colour map (no bases)
        o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
        first = None
        for opts in ({}, {"light_pool": 32}, {"light_base_pool": 32}, {"light_nest_pool": 0}, {"light_pool": 32, "light_base_pool": 32, "light_nest_pool": 0},
                     {"light_pool": 64, "chunk_spp": 4, "tile_log2": 1}):
            rgb, lin, st = gpu_render(sc, opts=opts)
            assert_parity(rgb, lin, o_rgb, o_lin, f"3 lights, general map {general_map}, {opts}", atol=pooled_atol(16))
            assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (opts, st["segments"])
            first = first if first is not None else (rgb, lin)
            assert np.array_equal(rgb, first[0]) and np.array_equal(lin, first[1]), opts
            if opts.get("light_pool") == 32 or (opts.get("light_base_pool") == 32 and not general_map):
                assert st["segments_repeated"] > 0, (opts, st["segments_repeated"])    # the exhausted pool was really met
            print(f"3 lights general_map={general_map} {opts}: kernel {st['kernel_ms']:.3f} ms, repeated {st['segments_repeated']}")
    # what the automatic sizing gives: the reference's test scene (7 spheres, one light) has room for a base per lane and 896 frames;
    # the cover scene + one light keeps its tables in LDS beside pools of at least 1.2 x the expected demand
    import json as _json
    sc1 = load_scene("test")
    gs = pkg.hip.HipScene(sc1.ptr, 0)
    fb = torch_cuda.zeros((600, 800, 3), dtype=torch_cuda.uint8, device="cuda:0")
    gs.render(fb.data_ptr(), 0, None, torch_cuda.cuda.current_stream().cuda_stream); gs.wait()
    assert gs.query("lds_tables") == 1 and gs.query("light_pool_slots") >= 512 and gs.query("light_base_slots") == 1024, (gs.query("light_pool_slots"), gs.query("light_base_slots"))
    assert gs.query("lds_bytes") <= 160 * 1024
    gs.close()
    cfg = _json.load(open(os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")))
    cfg.update(width=96, height=64, samples_per_pixel=2)
    cfg["objects"].append({"center": {"x": 0.0, "y": 30.0, "z": 10.0}, "radius": 8.0, "material": {"Light": {}}})
    sc = host.Scene.loads(_json.dumps(cfg))
    gs = pkg.hip.HipScene(sc.ptr, 0)
    fb = torch_cuda.zeros((64, 96, 3), dtype=torch_cuda.uint8, device="cuda:0")
    gs.render(fb.data_ptr(), 0, None, torch_cuda.cuda.current_stream().cuda_stream); st = gs.wait()
    print("lit cover pools:", gs.query("light_pool_slots"), gs.query("light_base_slots"), "lds", gs.query("lds_bytes"))
    assert gs.query("lds_tables") == 1 and gs.query("light_pool_slots") >= 1.2 * 66 and gs.query("light_base_slots") >= 1.2 * 0.16 * 1024
    assert st["segments_repeated"] == 0
    gs.close()


def test_lit_cover_scene_tables_beside_the_parked_light_state(gpu_render, oracle, abi, host):
    """lights in a gridded scene, two of them: every fifth hit of depth 0/1 samples them (with two lights the pool of
    light frames would be too small: one frame per lane, tables through L2).  Same frame as the oracle's, grid or brute
    force."""
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")))
    cfg.update(width=96, height=64, samples_per_pixel=8)
    cfg["objects"].append({"center": {"x": 0.0, "y": 30.0, "z": 10.0}, "radius": 8.0, "material": {"Light": {}}})
    cfg["objects"].append({"center": {"x": 3.0, "y": 2.5, "z": 2.0}, "radius": 0.4, "material": {"Light": {}}})
    sc = host.Scene.loads(json.dumps(cfg))
    assert len(sc.lights()) == 2 and sc.c.n_spheres == 486
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    for variant in (0, 1):
        rgb, lin, st = gpu_render(sc, variant=variant)
        assert_parity(rgb, lin, o_rgb, o_lin, f"lit cover variant {variant}", atol=pooled_atol(8))
        assert st["segments"] == o_st["segments"] - o_st["segments_discarded"]
    assert st["exact_tests"] == st["sphere_tests"]
    rgb, lin, st = gpu_render(sc, variant=0)
    assert st["grid_steps"] > 0 and st["exact_tests"] < 0.05 * st["sphere_tests"]
    # a small lit scene (tables AND parked frames in LDS) is what test_matches_oracle_and_golden[test_*] and
    # test_many_lights_nested_sampling render


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adversarial_spheres_on_the_gpu(gpu_render, oracle, abi, host, seed):
    """sphere records no JSON file can carry but the C ABI can: NaN / +-inf / 1e300 / denormal / zero radii, NaN / inf /
    1e308 centres, coincident spheres — among a few hundred ordinary ones, so the grid is built around them (non-finite
    records go to the `large` list) and rays leave their surfaces with non-finite or astronomically large coordinates
    (the walk's fallback).  Grid walk, brute force and the oracle must agree: same NaN pixels, same bits elsewhere.
    (tools/fuzz/fuzz_tables.cpp runs thousands of such sets through the CPU build of the same code under ASan.)"""
    sc = adversarial_scene(host, seed)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    nan = np.isnan(o_lin)
    for variant in (0, 1):
        rgb, lin, st = gpu_render(sc, variant=variant)
        assert np.array_equal(np.isnan(lin), nan), variant
        assert np.abs(np.where(nan, 0.0, lin) - np.where(nan, 0.0, o_lin)).max() <= pooled_atol(2), variant
        assert np.abs(rgb.astype(int) - o_rgb.astype(int)).max() <= 1
        assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], variant
    assert st["exact_tests"] == st["sphere_tests"]
    rgb, lin, st = gpu_render(sc, variant=0)
    assert st["grid_steps"] > 0


def test_procedural_10k_spheres(gpu_render, oracle, abi, host):
    """BASELINE configs[4] world (~10 000 spheres) at a size the oracle finishes in seconds"""
    import procedural
    sc = host.Scene.loads(procedural.make_json(width=64, height=36, spp=2, half=50, seed=0))
    assert sc.c.n_spheres == 10001
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    rgb, lin, st = gpu_render(sc)
    assert_parity(rgb, lin, o_rgb, o_lin, "10k spheres", atol=pooled_atol(2))
    assert st["segments"] == o_st["segments"]
    # the grid does its job: a handful of exact tests per segment instead of 10 001
    assert st["grid_steps"] > 0 and st["exact_tests"] < 40 * st["segments"]


def test_more_than_65535_spheres(gpu_render, oracle, abi, host):
    """any object count is accepted (the reference's Vec<Sphere> has no limit): above 65 535 spheres the packed cell tables
    (u16 item lists) cannot name a sphere and the scene takes the WIDE tables — 32-bit item lists, the kernel's wide
    instantiations, tables in L2.  The oracle's frame, the brute-force variant's bits, and a walk instead of 66 001 tests
    per segment (what such a scene cost until round 5)."""
    from fuzz_worlds import big_flat_world_json
    n = 66000
    sc = host.Scene.loads(big_flat_world_json(n, np.random.default_rng(3), width=16, height=10))
    assert sc.c.n_spheres == n + 1
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    q = {}
    rgb, lin, st = gpu_render(sc, query=q)
    assert q["grid_wide"] == 1 and q["grid_large"] <= 8 and q["grid_items"] >= n
    assert_parity(rgb, lin, o_rgb, o_lin, "66001 spheres", atol=pooled_atol(2))
    assert st["segments"] == o_st["segments"] and st["grid_steps"] > 0 and st["exact_tests"] < 30 * st["segments"]
    b_rgb, b_lin, b_st = gpu_render(sc, variant=1)
    assert np.array_equal(rgb, b_rgb) and np.array_equal(lin, b_lin) and b_st["exact_tests"] == b_st["sphere_tests"]


def test_a_cell_with_more_items_than_the_packed_word_counts(gpu_render, oracle, abi, host):
    """4 300 nearly coincident spheres in one cell (the packed cell word counts 4 095): wide tables, the oracle's frame, the
    brute-force variant's bits"""
    from fuzz_worlds import crowded_cell_world_json
    sc = host.Scene.loads(crowded_cell_world_json())
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    q = {}
    rgb, lin, st = gpu_render(sc, query=q)
    assert q["grid_wide"] == 1 and q["grid_large"] <= 8
    assert_parity(rgb, lin, o_rgb, o_lin, "crowded cell", atol=pooled_atol(2))
    assert st["segments"] == o_st["segments"] and st["exact_tests"] < st["sphere_tests"]
    b_rgb, b_lin, _ = gpu_render(sc, variant=1)
    assert np.array_equal(rgb, b_rgb) and np.array_equal(lin, b_lin)


def test_200k_spheres_at_speed(gpu_render, host):
    """2 x 10^5 spheres (three times the packed format's limit) at the cover scene's density, 640 x 360, spp 16: the frame takes
    milliseconds, not the minutes of a full scan (2 x 10^5 tests per segment); printed for the record.  (A FLAT world of this size
    is the grid's worst case: 256 cells per axis — the bound of the f32 walk's error analysis — leave 3 spheres per cell.)"""
    from fuzz_worlds import big_flat_world_json
    n = 200000
    sc = host.Scene.loads(big_flat_world_json(n, np.random.default_rng(5), width=640, height=360, spp=16, depth=50, half=224.0))
    q = {}
    rgb, _, st = gpu_render(sc, want_linear=False, frames=2, query=q)
    print(f"\n200k spheres 640x360 spp16: kernel {st['kernel_ms']:.2f} ms, {st['samples'] / st['kernel_ms'] / 1e3:.0f} Msamples/s, "
          f"{st['exact_tests'] / st['segments']:.2f} exact tests/segment, {st['grid_steps'] / st['segments']:.2f} steps/segment, grid {q}")
    assert q["grid_wide"] == 1 and st["exact_tests"] < 30 * st["segments"] and st["kernel_ms"] < 200.0
    assert rgb.std() > 5      # (a picture: sky, ground, spheres)


def test_wide_tables_render_the_packed_tables_frame(pkg, gpu_render, load_scene, monkeypatch):
    """The wide format is another encoding of the same grid: the cover scene through librt_hip_probe.so with RT_GRID_WIDE=1
    (the kernel's wide instantiation, tables in L2) gives the product's frame bit for bit, and its counters."""
    sc = load_scene("cover", 150, 100, 4, 50)
    rgb, lin, st = gpu_render(sc)
    monkeypatch.setenv("RT_GRID_WIDE", "1")
    q = {}
    w_rgb, w_lin, w_st = gpu_render(sc, library=pkg.hip.probe_lib(), query=q)
    assert q["grid_wide"] == 1
    assert np.array_equal(rgb, w_rgb) and np.array_equal(lin, w_lin)
    assert all(st[k] == w_st[k] for k in ("segments", "exact_tests", "grid_steps"))


@pytest.mark.parametrize("kind", range(6))
def test_wide_tables_on_the_fuzz_worlds(pkg, gpu_render, host, monkeypatch, kind):
    """fuzz worlds (mixed materials, two lights, hollow shells, a camera inside glass) through the wide kernels: the
    product's frame and counters, and the brute-force variant's frame"""
    from fuzz_worlds import fuzz_world_json
    sc = host.Scene.loads(fuzz_world_json(np.random.default_rng(3000 + kind), kind))
    rgb, lin, st = gpu_render(sc)
    monkeypatch.setenv("RT_GRID_WIDE", "1")
    q = {}
    w_rgb, w_lin, w_st = gpu_render(sc, library=pkg.hip.probe_lib(), query=q)
    assert q["grid_wide"] == 1
    assert np.array_equal(rgb, w_rgb) and np.array_equal(lin, w_lin)
    assert all(st[k] == w_st[k] for k in ("segments", "exact_tests", "grid_steps"))
    b_rgb, b_lin, _ = gpu_render(sc, library=pkg.hip.probe_lib(), variant=1)
    assert np.array_equal(w_rgb, b_rgb) and np.array_equal(w_lin, b_lin)


def test_host_buffer_entry_point(pkg, gpu_render, load_scene):
    """rt_render_rgb8 (host buffers in/out, the drop-in for render()'s loop) == device API"""
    sc = load_scene("cover", 80, 50, 2, 50)
    rgb, _, _ = gpu_render(sc)
    out, st = pkg.hip.render_rgb8(sc.ptr)
    assert np.array_equal(out, rgb) and st["kernel_ms"] > 0 and st["frame_ms"] >= st["kernel_ms"]


def test_cli_contract(tmp_path, gpu_render, load_scene):
    """main.rs:7-20: argv, the two stdout lines, PNG output; usage line + exit 0 on bad argc"""
    from PIL import Image
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg1_test_800x600_spp16.json")))
    cfg.update(width=64, height=48, samples_per_pixel=4)
    p = tmp_path / "s.json"
    p.write_text(json.dumps(cfg))
    out = tmp_path / "o.png"
    r = subprocess.run([exe, str(p), str(out)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "" and lines[1] == f"Rendering {out}" and lines[2].startswith("Frame time: ") and lines[2].endswith("ms")
    sc = load_scene(str(p))
    rgb, _, _ = gpu_render(sc)
    assert np.array_equal(np.asarray(Image.open(out)), rgb)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("Usage: ") and "<config_file> <output_file>" in r.stdout
    r = subprocess.run([exe, "/nonexistent.json", str(out)], capture_output=True, text=True)
    assert r.returncode == 101 and "Unable to read config file." in r.stderr


def _orbit_cameras(host, sc, n, deg):
    """the camera vectors (origin, lower-left, horizontal, vertical) of frames 0..n-1 of `--orbit deg`: look_from turned about
    vup around look_at (Rodrigues), then Camera::new (camera.rs:45-77) — the CLI's orbit_camera restated"""
    import math
    cam = (C.c_double * 11)()
    host.lib().rt_scene_camera.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    host.lib().rt_scene_camera.restype = None
    host.lib().rt_scene_camera(sc._h, cam)
    lf, la, up = list(cam[0:3]), list(cam[3:6]), list(cam[6:9])
    kl = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    k = [u / kl for u in up]
    cams = []
    for f in range(n):
        th = deg * f * (3.14159265358979323846264338327950288 / 180.0)
        c, s_ = math.cos(th), math.sin(th)
        v = [lf[i] - la[i] for i in range(3)]
        kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
        kx = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
        frm = [la[i] + v[i] * c + kx[i] * s_ + k[i] * kv * (1.0 - c) for i in range(3)]
        out = (C.c_double * 13)()
        host.lib().rt_camera_derive((C.c_double * 3)(*frm), (C.c_double * 3)(*la), (C.c_double * 3)(*up), cam[9], cam[10], out)
        cams.append((list(out[0:3]), list(out[3:6]), list(out[6:9]), list(out[9:12])))
    return cams


def _oracle_with_camera(oracle, abi, sc, cam):
    """the ORACLE's frame of the scene seen through `cam` (its RtScene camera fields overwritten, then restored)"""
    keep = [list(sc.c.cam_origin), list(sc.c.cam_lower_left), list(sc.c.cam_horizontal), list(sc.c.cam_vertical)]
    try:
        for i in range(3):
            sc.c.cam_origin[i], sc.c.cam_lower_left[i], sc.c.cam_horizontal[i], sc.c.cam_vertical[i] = cam[0][i], cam[1][i], cam[2][i], cam[3][i]
        return oracle.render(abi, sc.ptr)
    finally:
        for i in range(3):
            sc.c.cam_origin[i], sc.c.cam_lower_left[i], sc.c.cam_horizontal[i], sc.c.cam_vertical[i] = keep[0][i], keep[1][i], keep[2][i], keep[3][i]


@pytest.mark.parametrize("anim_env", [{}, {"RT_GPUS": "3", "RT_GPUS_EMULATE": "1"}, {"RT_ANIM": "frames", "RT_GPUS": "2", "RT_GPUS_EMULATE": "1"}])
def test_animation_driver(tmp_path, pkg, host, oracle, abi, torch_cuda, load_scene, anim_env):
    """`raytracer <config> <prefix> --frames N --orbit DEG` (the reference's anim/frame_%03d.png workflow, README.md:43-57,
    main.rs:17): the scene stays resident, only the camera moves (rt_hip_set_camera / rt_hip_group_set_camera).  Every frame's
    PNG is checked against the ORACLE rendering the scene through that frame's camera (camera.rs:45-84) — and the same
    moved-camera frame rendered through the device API (linear radiance: the full parity bar) and through a 3-rank group."""
    from PIL import Image
    torch = torch_cuda
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg1_test_800x600_spp16.json")))
    W, H, SPP = 72, 54, 3
    cfg.update(width=W, height=H, samples_per_pixel=SPP)
    p = tmp_path / "s.json"
    p.write_text(json.dumps(cfg))
    prefix = tmp_path / "frame"
    r = subprocess.run([exe, str(p), str(prefix), "--frames", "3", "--orbit", "25"], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RT_STATS="1", **anim_env))
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("\nRendering ") == 3 and r.stdout.count("Frame time: ") == 3
    rep = json.loads([l for l in r.stderr.splitlines() if l.startswith('{"animation"')][-1])
    assert rep["frames"] == 3 and rep["frames_per_s"] > 0 and len(rep["kernel_ms"]) == 3 and len(rep["png_ms"]) == 3
    assert all(k > 0 for k in rep["kernel_ms"]) and all(k > 0 for k in rep["png_ms"])
    sc = load_scene(str(p))
    cams = _orbit_cameras(host, sc, 3, 25.0)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    rgb_d = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    lin_d = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    grp = None
    if not anim_env:
        os.environ["RT_GPUS_EMULATE"] = "1"
        try:
            grp = pkg.hip.HipGroup(sc.ptr, 3)
        finally:
            del os.environ["RT_GPUS_EMULATE"]
    frames = []
    for f in range(3):
        o_rgb, o_lin, o_st = _oracle_with_camera(oracle, abi, sc, cams[f])
        gs.set_camera(*cams[f])
        gs.render(rgb_d.data_ptr(), lin_d.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        st = gs.wait()
        rgb = rgb_d.cpu().numpy()
        # the moved-camera frame against the oracle: linear radiance, RGB8, path count
        assert_parity(rgb, lin_d.cpu().numpy(), o_rgb, o_lin, f"frame {f} (rt_hip_set_camera)", atol=pooled_atol(SPP), flip_frac=2e-3)
        assert st["samples"] == W * H * SPP and st["segments"] == o_st["segments"] - o_st["segments_discarded"]
        # the CLI's PNG of that frame: the same bytes, hence the oracle's within the RGB8 bar
        got = np.asarray(Image.open(f"{prefix}_{f:03d}.png"))
        assert np.array_equal(got, rgb), f"frame {f}: PNG differs from the device API's frame"
        d = np.abs(got.astype(np.int16) - o_rgb.astype(np.int16))
        assert d.max() <= 1 and int((d != 0).sum()) <= max(2, int(2e-3 * d.size)), f"frame {f}: PNG vs oracle"
        if grp is not None:   # rt_hip_group_set_camera, 3 emulated ranks: the same frame, hence the oracle's
            grp.set_camera(*cams[f])
            g_rgb, g_st = grp.render_to_host()
            assert np.array_equal(g_rgb, rgb), f"frame {f}: 3-rank group after rt_hip_group_set_camera"
            assert g_st["segments"] == o_st["segments"] - o_st["segments_discarded"]
        frames.append(rgb)
    gs.close()
    if grp is not None:
        grp.close()
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])  # the camera did move


def _check_rows_against_oracle(rgb, lin, oracle, abi, sc, rows, spp, what, x_range=None):
    """exact scanlines (or pixel windows of them) of a full-size frame against the oracle at full spp"""
    worst = 0.0
    for y in rows:
        o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr, abi.RtRowTiles(1, y, 1 << 20), x_range=x_range)
        x0, x1 = x_range if x_range else (0, sc.c.width)
        err, _ = assert_parity(rgb[y:y + 1, x0:x1], lin[y:y + 1, x0:x1], o_rgb[:, x0:x1], o_lin[:, x0:x1], f"{what} row {y}",
                               atol=pooled_atol(spp), flip_frac=2e-3)
        worst = max(worst, err)
    return worst


def test_full_size_headline_config_properties(gpu_render, oracle, abi, load_scene):
    """BASELINE configs[1] at FULL size (1200x800, spp 128, depth 50, 484 spheres), checked
    through size-independent properties: determinism, shard invariance, counter identities,
    and exact scanlines against the oracle."""
    sc = load_scene("cover")
    c = sc.c
    assert (c.width, c.height, c.samples_per_pixel, c.max_depth, c.n_spheres) == (1200, 800, 128, 50, 484)
    rgb, lin, st = gpu_render(sc)
    print(f"full config kernel_ms={st['kernel_ms']:.2f} segments/sample={st['segments'] / st['samples']:.3f} "
          f"exact tests/segment={st['exact_tests'] / st['segments']:.2f}")
    assert st["samples"] == 1200 * 800 * 128 and st["sphere_tests"] == st["segments"] * 484
    assert 2.0 < st["segments"] / st["samples"] < 3.5  # SURVEY §8d measured ~2.66
    rgb2, lin2, st2 = gpu_render(sc)
    assert np.array_equal(rgb, rgb2) and np.array_equal(lin, lin2) and st2["segments"] == st["segments"]
    # the per-XCD tile queues (on by default at this size; three frames: the depth-sorted per-XCD order kicks in) and
    # the single queue hand out the same frame, whatever the tile size
    for aff, tl, frames in ((0, None, 1), (1, None, 3), (1, 3, 3), (1, 1, 1), (0, 3, 1)):
        a_rgb, a_lin, a_st = gpu_render(sc, tile_affinity=aff, tile_log2=tl, frames=frames)
        assert np.array_equal(a_rgb, rgb) and np.array_equal(a_lin, lin) and a_st["segments"] == st["segments"], (aff, tl)
    # shard invariance: rank 3 of 8 renders exactly its scanlines of the full frame
    t = abi.RtRowTiles(8, 3, 8)
    rows = abi.tiles_global_rows(800, t)
    s_rgb, s_lin, _ = gpu_render(sc, tiles=t)
    assert np.array_equal(s_rgb, rgb[rows]) and np.array_equal(s_lin, lin[rows])
    # the WHOLE frame against the oracle's whole frame at full spp (the 128 host threads of the GPU box take ~21 s):
    # radiance, RGB8, and the path count — every one of the 122.88 M samples traces the oracle's path
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    worst, flips = assert_parity(rgb, lin, o_rgb, o_lin, "cfg2 whole frame", atol=pooled_atol(128), flip_frac=5e-4)
    assert st["segments"] == o_st["segments"] - o_st["segments_discarded"] and o_st["segments_discarded"] == 0
    print(f"cfg2 full size: WHOLE frame (800 scanlines, 122.88 M samples) vs oracle, max |dlin| {worst:.2e}, rgb8 flips {flips} of {rgb.size}")
    # image statistics sanity: top rows are sky gradient, bottom rows ground
    assert lin[:40].mean() > lin[-40:].mean()


def test_full_size_cfg1_test_scene(gpu_render, oracle, abi, load_scene):
    """BASELINE configs[0] at FULL size (test_scene 800x600, spp 16, depth 8: a Light, earth / moon textures, sky texture,
    Metal, hollow Glass with a negative radius): the WHOLE frame against the oracle's whole frame — radiance, RGB8, path
    count (minus the light loops the reference discards), no out-of-range texel."""
    sc = load_scene("test")
    c = sc.c
    assert (c.width, c.height, c.samples_per_pixel, c.max_depth, c.n_spheres) == (800, 600, 16, 8, 7) and len(sc.lights()) == 1
    rgb, lin, st = gpu_render(sc)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    err, flips = assert_parity(rgb, lin, o_rgb, o_lin, "cfg1 whole frame", atol=pooled_atol(16), flip_frac=5e-4)
    assert st["segments"] == o_st["segments"] - o_st["segments_discarded"] and o_st["segments_discarded"] > 0
    assert st["tex_oob"] == 0 == o_st["tex_oob"] and st["samples"] == 800 * 600 * 16
    print(f"cfg1 full size: whole frame vs oracle, max |dlin| {err:.2e}, rgb8 flips {flips}, kernel {st['kernel_ms']:.2f} ms")


def test_full_size_cfg3_textured_4k(gpu_render, oracle, abi, load_scene):
    """BASELINE configs[2] at FULL size: cover world at 3840x2160, spp 1024, earth / moon textures on the three big
    spheres + beach sky texture (the texture-fetch path: sphere_uv's atan2, get_albedo, sky lookup).  Whole frame on
    the GPU; exact 4K scanlines against the oracle at the full 1024 spp — through the sky, the textured spheres
    (rows ~900-1500) and the ground; determinism; no out-of-range texel."""
    sc = load_scene("cover4k_tex")
    c = sc.c
    assert (c.width, c.height, c.samples_per_pixel, c.max_depth, c.n_spheres) == (3840, 2160, 1024, 50, 484)
    assert c.sky_mode == abi.RT_SKY_TEXTURE and c.n_textures >= 2
    rgb, lin, st = gpu_render(sc)
    print(f"cfg3 full size kernel_ms={st['kernel_ms']:.1f} Msamples/s={st['samples'] / st['kernel_ms'] / 1e3:.0f} "
          f"segments/sample={st['segments'] / st['samples']:.3f}")
    assert st["samples"] == 3840 * 2160 * 1024 and st["tex_oob"] == 0
    # 32 whole 4K scanlines: sky texture, horizon, then every ~28 rows through the three textured r = 1 spheres (rows
    # ~640-1520: poles, seam of the u wrap behind the h_offset rotation, limb), the small spheres and the ground
    rows = (40, 300, 560, 640, 668, 700, 760, 820, 880, 940, 1000, 1040, 1080, 1120, 1160, 1200, 1240, 1280, 1320, 1360, 1400, 1440, 1480,
            1520, 1600, 1700, 1800, 1900, 2000, 2100, 2140, 2159)
    assert len(rows) == 32
    worst = _check_rows_against_oracle(rgb, lin, oracle, abi, sc, rows, 1024, "cfg3")
    print(f"cfg3 full size: {len(rows)} scanlines x 3840 px x 1024 spp vs oracle, max |dlin| {worst:.2e}")
    # shard invariance at this size: rank 5 of 8 (2-row interleave, the group's layout) renders its scanlines' bits
    t = abi.RtRowTiles(2, 5, 8)
    rows = abi.tiles_global_rows(2160, t)
    s_rgb, _, s_st = gpu_render(sc, tiles=t, want_linear=False)
    assert np.array_equal(s_rgb, rgb[rows]) and s_st["samples"] == len(rows) * 3840 * 1024


def test_full_size_cfg5_10k_spheres_4k(gpu_render, oracle, abi, host):
    """BASELINE configs[4] at FULL size: procedural 10 001-sphere world, 3840x2160, spp 2048 (tables too big for
    LDS: the LDS_TABLES = false instantiation gathers from L2).  Whole frame on the GPU; pixel windows of scanlines
    against the oracle's brute force over all 10 001 spheres at the full 2048 spp."""
    import procedural
    sc = host.Scene.loads(procedural.make_json(width=3840, height=2160, spp=2048, half=50, seed=0))
    assert sc.c.n_spheres == 10001
    rgb, lin, st = gpu_render(sc)
    print(f"cfg5 full size kernel_ms={st['kernel_ms']:.1f} Msamples/s={st['samples'] / st['kernel_ms'] / 1e3:.0f} "
          f"exact/segment={st['exact_tests'] / st['segments']:.2f} steps/segment={st['grid_steps'] / st['segments']:.2f}")
    assert st["samples"] == 3840 * 2160 * 2048 and st["grid_steps"] > 0 and st["exact_tests"] < 40 * st["segments"]
    worst = 0.0
    windows = ((30, 1900), (520, 100), (700, 300), (760, 2500), (900, 3600), (1000, 1200), (1100, 1900), (1200, 640), (1300, 1800), (1400, 3000),
               (1500, 0), (1650, 2200), (1800, 1000), (2000, 3400), (2100, 1700), (2159, 3648))
    assert len(windows) == 16
    for y, x0 in windows:
        worst = max(worst, _check_rows_against_oracle(rgb, lin, oracle, abi, sc, (y,), 2048, "cfg5", x_range=(x0, x0 + 192)))
    print(f"cfg5 full size: {len(windows)} windows x 192 px x 2048 spp vs oracle (10 001 spheres brute force), max |dlin| {worst:.2e}")


@pytest.mark.parametrize("radii", ["loguniform", "bimodal"])
def test_mixed_radius_10k_sphere_worlds(gpu_render, oracle, abi, host, radii):
    """SURVEY §8 f2 outside BASELINE's sphere distribution (round-4 verdict next #7): 10^4 spheres whose radii span two
    decades — log-uniform in [0.05, 5], and 95 % r = 0.05 + 5 % r = 3.0 — on the configs[4] lattice stretched by 4
    (scenes/procedural.py).  A single-level uniform grid is not made for these (a cell sized for the small spheres is crossed by
    every big one): the table builder coarsens the grid and keeps the 8 biggest spheres in the `large` list.  The frame must be
    the oracle's (brute force over all 10^4 spheres: pixel windows of scanlines at full spp) and the brute-force variant's
    bit for bit; the speed number and the exact tests per segment are printed (the bench line carries them too)."""
    import procedural
    sc = host.Scene.loads(procedural.make_json(width=640, height=360, spp=32, half=50, seed=0, radii=radii))
    assert 9900 < sc.c.n_spheres <= 10001
    rgb, lin, st = gpu_render(sc)
    assert st["grid_steps"] > 0 and st["exact_tests"] < 40 * st["segments"]
    worst = 0.0
    for y, x0 in ((20, 100), (120, 400), (200, 0), (250, 250), (300, 480), (359, 320)):
        worst = max(worst, _check_rows_against_oracle(rgb, lin, oracle, abi, sc, (y,), 32, f"mixed radii {radii}", x_range=(x0, x0 + 160)))
    small = host.Scene.loads(procedural.make_json(width=160, height=90, spp=4, half=50, seed=0, radii=radii))
    g_rgb, g_lin, g_st = gpu_render(small, variant=0)
    b_rgb, b_lin, b_st = gpu_render(small, variant=1)
    assert np.array_equal(g_rgb, b_rgb) and np.array_equal(g_lin, b_lin) and g_st["segments"] == b_st["segments"]
    big = host.Scene.loads(procedural.make_json(width=1920, height=1080, spp=128, half=50, seed=0, radii=radii))
    ks = [gpu_render(big, want_linear=False)[2] for _ in range(2)]
    k = min(x["kernel_ms"] for x in ks)
    print(f"mixed radii {radii}: {sc.c.n_spheres} spheres, 6 windows vs oracle max |dlin| {worst:.2e}; 1920x1080 spp 128: {k:.1f} ms = {ks[0]['samples'] / k / 1e3:.0f} Msamples/s, "
          f"segments/sample {ks[0]['segments'] / ks[0]['samples']:.2f}, exact tests/segment {ks[0]['exact_tests'] / ks[0]['segments']:.2f}, grid steps/segment {ks[0]['grid_steps'] / ks[0]['segments']:.2f}")
    assert ks[0]["exact_tests"] / ks[0]["segments"] < 30.0     # (above 30 a second grid level for the medium spheres would be the next step: it is not)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_group_in_library_sharding_is_bit_identical(pkg, gpu_render, load_scene, world):
    """rt_hip_group_* (multi-GPU inside librt_hip.so: a host thread + stream per rank, interleaved 2-row tiles, gather
    buffer, de-interleave kernel, one D2H), with RT_GPUS_EMULATE=1 so that the ranks share this box's one GPU: the frame,
    the path count and the sample count are those of the single launch, for cover (no lights) and test_scene (lights,
    textures), several frames in a row."""
    for scene, w, h, spp, depth in (("cover", 100, 67, 3, 50), ("test", 64, 49, 3, 8)):
        sc = load_scene(scene, w, h, spp, depth)
        rgb, _, st = gpu_render(sc, want_linear=False)
        grp = _with_env({"RT_GPUS_EMULATE": "1"}, lambda: pkg.hip.HipGroup(sc.ptr, world))
        assert grp.size == world
        for _ in range(3):
            out, gst = grp.render_to_host()
            assert np.array_equal(out, rgb), (scene, world)
            assert gst["n_gpus_used"] == world and gst["samples"] == st["samples"] and gst["segments"] == st["segments"]
            assert gst["kernel_ms"] > 0 and gst["frame_ms"] >= gst["kernel_ms"]
        grp.set_option("seed", 5)
        out2, _ = grp.render_to_host()
        assert not np.array_equal(out2, rgb)
        grp.close()


def test_full_size_cfg4_through_the_8_rank_group(pkg, gpu_render, oracle, abi, load_scene):
    """BASELINE configs[3] at FULL size (3840x2160, spp 512, textured): the in-library group with 8 ranks (sharing this
    box's GPU) against the single launch — byte-identical frame, same path count; two frames (the second with the queue
    order learnt from the first)."""
    sc = load_scene("scenes/cfg4_cover_4k_textured_spp512.json")
    assert (sc.c.width, sc.c.height, sc.c.samples_per_pixel) == (3840, 2160, 512)
    rgb, _, st = gpu_render(sc, want_linear=False)
    grp = _with_env({"RT_GPUS_EMULATE": "1"}, lambda: pkg.hip.HipGroup(sc.ptr, 8))
    for _ in range(2):
        out, gst = grp.render_to_host()
        assert np.array_equal(out, rgb)
        assert gst["n_gpus_used"] == 8 and gst["samples"] == st["samples"] == 3840 * 2160 * 512 and gst["segments"] == st["segments"]
    print(f"cfg4 full size: single launch {st['kernel_ms']:.1f} ms; 8 emulated ranks on one GPU: slowest rank {gst['kernel_ms']:.1f} ms, frame {gst['frame_ms']:.1f} ms")
    grp.close()
    # ... and that frame against the ORACLE at the full 512 spp: four whole 4K scanlines (sky, the textured spheres incl.
    # the seam of the u wrap, the small spheres, the ground) — rows of ranks 6, 5, 4 and 7 of the 2-row interleave
    _, lin, _ = gpu_render(sc)
    rows = (300, 1002, 1320, 2159)
    assert sorted({(y // 2) % 8 for y in rows}) == [4, 5, 6, 7]
    worst = _check_rows_against_oracle(out, lin, oracle, abi, sc, rows, 512, "cfg4")
    print(f"cfg4 full size: {len(rows)} scanlines x 3840 px x 512 spp of the 8-rank frame vs oracle, max |dlin| {worst:.2e}")


def test_group_gather_through_rccl_one_rank(pkg, gpu_render, load_scene):
    """the RCCL leg of the group (dlopen, ncclCommInitAll, in-place ncclGather inside a group call, de-interleave
    kernel) with the only communicator a 1-GPU box allows: one rank (RT_GATHER_SELFTEST=1)"""
    sc = load_scene("cover", 96, 40, 2, 50)
    rgb, _, _ = gpu_render(sc, want_linear=False)
    for transport in ("rccl", "peer"):
        grp = _with_env({"RT_GATHER_SELFTEST": "1", "RT_GATHER": transport}, lambda: pkg.hip.HipGroup(sc.ptr, 1))
        for _ in range(2):
            out, gst = grp.render_to_host()
            assert np.array_equal(out, rgb), transport
            assert gst["gather_ms"] >= 0.0
        grp.close()


def test_group_transport_fallback_never_costs_the_frame(pkg, gpu_render, load_scene):
    """The first 8-GPU run happens without a builder watching: whatever RCCL cannot do there, the group must still deliver the
    frame — on peer copies — and say so.  On the one-GPU box (a one-rank communicator, RT_GATHER_SELFTEST=1): the library that
    does not load (RT_RCCL_LIB), a self-test gather that delivers wrong bytes, and a gather that fails to enqueue in the
    SECOND frame (the switch happens mid-stream, that frame's tiles are re-sent) all end on transport "peer" with
    transport_fallback set and a reason, and every frame — blocking and pipelined — is the single launch's bytes."""
    sc = load_scene("cover", 96, 40, 2, 50)
    rgb, _, _ = gpu_render(sc, want_linear=False)
    base = {"RT_GATHER_SELFTEST": "1", "RT_GATHER": "rccl"}
    cases = (("healthy", {}, "rccl", ""), ("library", {"RT_RCCL_LIB": "/nonexistent/librccl.so"}, "peer", "cannot load RCCL"),
             ("selftest", {"RT_RCCL_INJECT": "selftest"}, "peer", "self-test gather delivered"), ("gather", {"RT_RCCL_INJECT": "gather"}, "peer", "ncclGather"))
    for name, extra, transport, reason in cases:
        def run():
            # (the fault-injection hooks exist in librt_hip_probe.so only — the same sources + -DRT_TEST_PROBES)
            grp = pkg.hip.HipGroup(sc.ptr, 1, library=pkg.hip.probe_lib() if "RT_RCCL_INJECT" in extra else None)
            infos = [grp.info()]
            frames = []
            for _ in range(3):                  # (the injected gather failure hits the second submit of the group)
                out, st = grp.render_to_host()
                frames.append(out)
            bufs = [np.zeros_like(rgb) for _ in range(3)]
            grp.submit(bufs[0]); grp.submit(bufs[1]); grp.collect(); grp.submit(bufs[2]); grp.collect(); grp.collect()
            infos.append(grp.info())
            ranks = grp.ranks()
            grp.close()
            return infos, frames + bufs, ranks
        infos, frames, ranks = _with_env(dict(base, **extra), run)
        for k, f in enumerate(frames):
            assert np.array_equal(f, rgb), (name, k)
        first, last = infos
        assert last["transport"] == transport and last["transport_fallback"] == (transport == "peer") and reason in last["fallback_reason"], (name, last)
        if name == "gather":
            assert first["transport"] == "rccl" and not first["transport_fallback"]      # it switched in the second frame, not before
        if name in ("library", "selftest"):
            assert first["transport"] == "peer" and first["rccl_comms"] == 0
        assert len(ranks) == 1 and ranks[0]["device"] == 0 and ranks[0]["kernel_ms"] > 0 and ranks[0]["peer_to_root"] == 1 and len(ranks[0]["pci_bus_id"]) >= 7, ranks
        print(f"group transport case {name}: {last['transport']} fallback={last['transport_fallback']} reason={last['fallback_reason']!r} rank0={ranks[0]}")
    # ... and the PRODUCT library does not read RT_RCCL_INJECT: a stray variable cannot switch its transport

    def product_run():
        grp = pkg.hip.HipGroup(sc.ptr, 1)
        for _ in range(3):
            out, _ = grp.render_to_host()
            assert np.array_equal(out, rgb)
        info = grp.info()
        grp.close()
        return info
    for inj in ("selftest", "gather"):
        info = _with_env(dict(base, RT_RCCL_INJECT=inj), product_run)
        assert info["transport"] == "rccl" and not info["transport_fallback"], (inj, info)


@pytest.mark.parametrize("world,env,bar_us", [(1, {}, 150.0), (8, {"RT_GPUS_EMULATE": "1"}, 400.0)])
def test_group_submit_into_a_pageable_buffer_does_not_block(pkg, load_scene, world, env, bar_us):
    """rt_hip_group_submit(out) with an ordinary (pageable) host buffer used to block until the frame was rendered — an
    asynchronous copy into pageable memory is synchronous in HIP — so the two-deep pipeline degenerated for exactly the call a
    drop-in host makes (submit returned after 1 840 us, profiles/r04_run1_group_overhead.json).  The frame now leaves into
    a pinned staging buffer of the group and collect moves it on: submit returns within the host's enqueue time (bar: 150 us
    for one rank) while the kernel is still running, and the bytes are the blocking frame's."""
    sc = load_scene("cover", 600, 400, 16, 50)     # ~1 ms of kernel: a blocking submit would show
    grp = _with_env(env, lambda: pkg.hip.HipGroup(sc.ptr, world))
    want, st0 = grp.render_to_host()
    assert st0["kernel_ms"] > 0.3
    bufs = [np.zeros_like(want) for _ in range(3)]
    returns = []
    for rep in range(12):
        grp.submit(bufs[rep % 3])
        st = grp.collect()
        assert np.array_equal(bufs[rep % 3], want)
        returns.append(st["group_us"][4])
        assert st["group_us"][6] >= st["group_us"][4]
    grp.close()
    best = sorted(returns[2:])[len(returns[2:]) // 2]
    print(f"group of {world}: submit(out = pageable numpy) returns after {best:.0f} us (median; kernel {st0['kernel_ms']:.2f} ms); all: {[round(r) for r in returns]}")
    assert best <= bar_us and best < 0.5 * st0["kernel_ms"] * 1e3, (best, returns)


def test_group_rejects_more_gpus_than_visible(pkg, load_scene):
    sc = load_scene("cover", 16, 16, 1, 5)
    os.environ.pop("RT_GPUS_EMULATE", None)
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipGroup(sc.ptr, pkg.hip.device_count() + 1)
    assert e.value.code == pkg.abi.RT_ERR_INVALID


def test_cli_multi_gpu_env(tmp_path):
    """RT_GPUS=N through the CLI (single frame and animation): byte-identical PNGs to the one-GPU run"""
    from PIL import Image
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg1_test_800x600_spp16.json")))
    cfg.update(width=64, height=50, samples_per_pixel=3)
    p = tmp_path / "s.json"
    p.write_text(json.dumps(cfg))
    imgs = {}
    for g in (1, 4):
        env = dict(os.environ, RT_GPUS=str(g), RT_GPUS_EMULATE="1", RT_STATS="1")
        out = tmp_path / f"o{g}.png"
        r = subprocess.run([exe, str(p), str(out)], capture_output=True, text=True, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr
        stats = json.loads(r.stderr.strip().splitlines()[-1])
        assert stats["n_gpus"] == g and stats["setup_ms"] > 0 and stats["frame_ms"] >= stats["kernel_ms"]
        assert r.stdout.split("\n")[2].startswith("Frame time: ")
        imgs[g] = np.asarray(Image.open(out))
        # animations: 5 frames (the sharded mode pipelines them two deep over three host buffers), and — RT_ANIM=frames —
        # the frames distributed over the devices, each rendering whole frames: the same PNG bytes every way
        for mode in ("sharded", "frames"):
            r = subprocess.run([exe, str(p), str(tmp_path / f"a{g}{mode}"), "--frames", "5", "--orbit", "30"], capture_output=True, text=True, cwd=ROOT,
                               env=dict(env, RT_ANIM=mode))
            assert r.returncode == 0, r.stderr
            assert r.stdout.count("\nRendering ") == 5 and r.stdout.count("Frame time: ") == 5
            rep = json.loads(r.stderr.strip().splitlines()[-1])
            assert rep["animation"] == mode and rep["frames"] == 5 and rep["n_gpus"] == g and rep["frames_per_s"] > 0
            imgs[(g, mode)] = [np.asarray(Image.open(tmp_path / f"a{g}{mode}_{f:03d}.png")) for f in range(5)]
    assert np.array_equal(imgs[1], imgs[4])
    for key in ((4, "sharded"), (1, "frames"), (4, "frames")):
        assert all(np.array_equal(a, b) for a, b in zip(imgs[(1, "sharded")], imgs[key])), key
    assert not np.array_equal(imgs[(1, "sharded")][0], imgs[(1, "sharded")][4])
    r = subprocess.run([exe, str(p), str(tmp_path / "x.png")], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, RT_GPUS="64"))
    assert r.returncode == 101 and "device" in r.stderr    # more GPUs than the box has: refused, like any render failure


def test_scene_is_not_reentrant_across_streams(pkg, load_scene, torch_cuda):
    """rt_abi.h: one tile queue / counter block per RtHipScene — a launch on a second stream before rt_hip_wait is refused"""
    torch = torch_cuda
    sc = load_scene("cover", 600, 400, 64, 50)                 # (milliseconds of work per launch: the refusal below must not race the kernels' end)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    a = torch.zeros((400, 600, 3), dtype=torch.uint8, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    gs.render(a.data_ptr(), 0, None, s1.cuda_stream)
    gs.render(a.data_ptr(), 0, None, s1.cuda_stream)           # same stream, back to back: fine
    with pytest.raises(pkg.host.RtError) as e:
        gs.render(a.data_ptr(), 0, None, s2.cuda_stream)
    assert e.value.code == pkg.abi.RT_ERR_INVALID
    gs.wait()
    gs.render(a.data_ptr(), 0, None, s2.cuda_stream)           # after the wait the scene may move to another stream
    gs.wait()
    with pytest.raises(pkg.host.RtError):
        gs.set_option("samples_per_pixel", -1)
    with pytest.raises(pkg.host.RtError):
        gs.set_option("max_depth", 1 << 40)
    gs.close()


@pytest.mark.parametrize("force_rccl", [False, True, "gloo", "inject"])
def test_bench_line_contract(force_rccl):
    """`bench.py --full` prints ONE JSON line with the driver's keys (+ roofline / cpu_baseline / other_configs objects) and
    nothing else on stdout — also when an RCCL group is up (RT_BENCH_FORCE_COLLECTIVE: the N > 1 code path with one
    rank; RCCL's version banner must not reach stdout), where it also carries the one-frame latency, the rank /
    device census and the per-rank arrays — and when RCCL does NOT come up ("inject": its set-up raises; "gloo": forced):
    the run falls back to a host-staged gather over gloo, says so, and still delivers its line."""
    env = dict(os.environ, MASTER_PORT={False: "29561", True: "29562", "gloo": "29563", "inject": "29564"}[force_rccl])
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--cpu-row-stride", "200", "--full"]
    if force_rccl:
        env["RT_BENCH_FORCE_COLLECTIVE"] = "1"
        cmd.append("--no-other-configs")
    if force_rccl == "gloo":
        env["RT_BENCH_FORCE_TRANSPORT"] = "gloo"
    if force_rccl == "inject":
        env["RT_BENCH_INJECT_NCCL_FAILURE"] = "1"
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "Msamples/s" and d["higher_is_better"] is True
    assert "workload" in d["config"] and "BASELINE configs[1]" in d["config"]["workload"]
    samples = 1200 * 800 * 128
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "executed_f64", "algorithmic"):
        assert k in rf, k
    assert rf["bound"] == "valu" and 0 < rf["executed_f64"]["frac"] < 1 and rf["algorithmic"]["algorithmic_speedup"] > 10
    if rf["frac"] is not None:   # (a profiles/rNN_*pmc.json of this build is committed: executed basis, below 1 by construction)
        assert 0 < rf["frac"] <= 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 2e-3
        assert abs(rf["frac"] - rf["valu_issue_busy"] * rf["lane_utilisation"]) < 0.02
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    if force_rccl:
        healthy = force_rccl is True
        assert d["rccl_ranks"] == (1 if healthy else 0) and d["visible_gpus"] >= 1 and len(d["rank_devices"]) == 1
        assert d["transport"] == ("rccl" if healthy else "gloo-host") and d["transport_fallback"] == (not healthy)
        assert (d["transport_fallback_reason"] is None) == healthy
        if force_rccl == "inject":
            assert "injected" in d["transport_fallback_reason"]
        pr = d["per_rank"]
        assert len(pr["kernel_ms"]) == 1 and pr["kernel_ms"][0] > 0 and pr["samples_share"] == [1.0] and len(pr["pci_bus_id"]) == 1 and pr["peer_to_root"] == [1]
        assert d["frame_latency_ms"] >= d["kernel_ms"] * 0.9 and "other_configs" not in d
    else:
        oc = d["other_configs"]
        assert len(oc) == 4 and all(c["kernel_ms"] > 0 and c["msamples_per_s"] > 0 for c in oc)
        assert oc[3]["n_spheres"] == 10001 and "configs[2]" in oc[1]["config"]
        for c in oc:   # counters of a config (when committed) are priced on BOTH clocks: the counter passes' own and this run's
            if "counters_source" in c and "lane_slot_frac" in c:
                assert 0 < c["lane_slot_frac_on_this_runs_clock"] <= 1
                if "lane_slot_frac_on_counter_clock" in c:
                    assert c["lane_slot_frac"] == c["lane_slot_frac_on_counter_clock"] and c["counter_run_kernel_ms"] > 0
            assert "traffic" not in c   # (FETCH_SIZE / WRITE_SIZE are L2 misses, not HBM bytes: l2_miss_bytes + hbm_bytes_compulsory)
        # the animation workflow in fresh processes — frames/s disk to disk, moving-camera kernel times, PNG times
        an = d["animation"]
        assert len(an) == 2 and all("error" not in a for a in an), an
        for a in an:
            assert a["frames"] == 32 and a["pngs_on_disk"] == 32 and a["frames_per_s"] > 0 and len(a["kernel_ms_series"]) == 32
            assert a["kernel_ms_moving_camera"]["median"] > 0 and a["png_ms"]["median"] > 0 and a["bound_by"] in ("kernel", "png")
            assert 0 < a["overlap_efficiency"] <= 1.05
        assert an[0]["moving_over_steady"] > 0.8 and len(an[0]["same_views"]["frames"]) == 5


FULL_ONLY_KEYS = ("cpu_baseline", "parity_vs_oracle", "other_configs", "mixed_radius_worlds", "cli", "animation", "first_frame_kernel_ms",
                  "frame_ms_to_host_buffer", "frame_latency_ms", "n1_kernel_ms", "frame_identical_to_n1", "configs3_on_group")


def test_plain_bench_run_carries_only_the_timed_steps():
    """A plain `bench.py` run (no --full) sets up, warms up, times its steps and prints the line: the headline keys and the
    figures of the timed steps themselves, and none of what --full measures or checks after them."""
    env = dict(os.environ, MASTER_PORT="29565")
    env.pop("WORLD_SIZE", None)
    steps, warmup = 3, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600, env=env)
    wall_s = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "kernel_ms", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["dtype"] == "f64" and "error" not in d
    assert abs(d["value"] - 1200 * 800 * 128 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    assert [k for k in FULL_ONLY_KEYS if k in d] == []
    print(f"plain bench run: {wall_s:.1f} s wall, {wall_s - (steps + warmup) * d['ms_per_step'] * 1e-3:.1f} s outside its steps")


@pytest.mark.parametrize("kind", range(6))
def test_fuzz_worlds_grid_equals_bruteforce_on_the_gpu(gpu_render, hostsim, oracle, abi, host, kind):
    """The product kernel (grid walk) against the ORACLE on random worlds (mixed materials, lights, hollow shells,
    camera inside glass), against the same kernel running the reference's scan over every sphere (variant 1: same
    bits, same path count) and against the CPU build of the lane logic (same bits)."""
    rng = np.random.default_rng(1000 + kind)
    sc = host.Scene.loads(fuzz_world_json(rng, kind))
    a_rgb, a_lin, a_st = gpu_render(sc, variant=0)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    assert_parity(a_rgb, a_lin, o_rgb, o_lin, f"fuzz world {kind} vs oracle", atol=pooled_atol(sc.c.samples_per_pixel), flip_frac=1e-3)
    assert a_st["segments"] == o_st["segments"] - o_st["segments_discarded"], kind
    b_rgb, b_lin, b_st = gpu_render(sc, variant=1)
    assert a_st["segments"] == b_st["segments"], kind
    assert np.array_equal(a_lin, b_lin) and np.array_equal(a_rgb, b_rgb), kind
    h_rgb, h_lin, h_st = hostsim.render(sc.ptr, mode=3 + 16)
    assert int(h_st["segments"]) == a_st["segments"] and np.array_equal(h_lin, a_lin) and np.array_equal(h_rgb, a_rgb), kind
    if kind != 2:
        assert a_st["grid_steps"] > 0, "the world is expected to be gridded"


_RCCL_ONE_RANK = r'''
import os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, os.getcwd())
import __graft_entry__ as graft
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[1], RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)   # nccl == RCCL on ROCm
pkg = graft.load_package()
from rust_raytracer_amd import dist as rdist
sc = pkg.host.Scene.load("scenes/cfg2_cover_1200x800_spp128.json")
sc.c.width, sc.c.height, sc.c.samples_per_pixel = 96, 40, 2
W, H = 96, 40
stream = torch.cuda.current_stream()
pipe = rdist.FramePipeline(H, W, 0, 1, dev, force_collective=True)
frames, want = [], []
for i in range(5):
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.set_option("seed", i)                       # every frame differs
    ref = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    gs.render(ref.data_ptr(), 0, None, stream.cuda_stream); gs.wait()
    want.append(ref.cpu().numpy())
    buf, done = pipe.begin(i)
    if done is not None:
        frames.append(done.cpu().numpy())
    gs.render(buf.data_ptr(), 0, None, stream.cuda_stream)
    pipe.submit(i)                                 # asynchronous gather over RCCL
    gs.wait(); gs.close()
frames += [f.cpu().numpy() for f in pipe.drain()]
dist.barrier(); torch.cuda.synchronize()
assert len(frames) == 5
for i in range(5):
    assert np.array_equal(frames[i], want[i]), i
assert not np.array_equal(want[0], want[1])
dist.destroy_process_group()
print("RCCL_PIPELINE_OK")
'''


def test_frame_pipeline_through_rccl_one_rank(tmp_path):
    """bench.py's N > 1 machinery (double-buffered tiles, asynchronous `gather` on RCCL's stream,
    row permutation on the destination) with the only process group a 1-GPU box allows: one rank."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "rccl_one_rank.py"
    script.write_text(_RCCL_ONE_RANK)
    r = subprocess.run([sys.executable, str(script), str(port)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "RCCL_PIPELINE_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_bench_process_per_gpu_with_two_ranks_on_this_gpu():
    """What the driver's scaling run launches — `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` — with N = 2
    REAL processes on this box's one GPU (RT_BENCH_ALLOW_SHARED_DEVICE=1; RCCL refuses two ranks on one device, so the tiles
    take the host-staged gloo route — the fall-back the run would take on a node whose RCCL does not come up): every line of
    the world > 1 branch runs on a GPU — rendezvous, shards, the pipelined gathers, the blocking-frame latency, rank 0's N = 1
    reference, the reductions, the per-rank arrays — and rank 0 prints ONE line."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RT_BENCH_ALLOW_SHARED_DEVICE="1", RT_BENCH_FORCE_TRANSPORT="gloo")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "strong" and "error" not in d
    assert d["transport"] == "gloo-host" and d["transport_fallback"] is True and d["ranks_share_devices"] is True
    pr = d["per_rank"]
    assert len(pr["kernel_ms"]) == 2 and min(pr["kernel_ms"]) > 0 and abs(sum(pr["samples_share"]) - 1.0) < 1e-3
    assert len(pr["pinned_cpus"]) == 2 and all(c >= 0 for c in pr["pinned_cpus"])   # (each rank's host thread on its GPU's NUMA node when sysfs names one)
    samples = 1200 * 800 * 128
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    assert d["n1_kernel_ms"] > 0 and d["frame_latency_ms"] > 0 and d["segments_per_sample"] > 2.0
    _check_multi_gpu_line_extras(d, 2)
    print(f"two ranks on one GPU (gloo-host): {d['value']:.0f} Msamples/s, {d['ms_per_step']:.2f} ms/step, per-rank kernel {pr['kernel_ms']}, frame latency {d['frame_latency_ms']:.2f} ms")


def test_device_sphere_hit_matches_oracle_and_host_build(pkg, hostsim, oracle, abi, torch_cuda):
    """Sphere::hit pair by pair on the device (the kernel's own exact_hit_any_order) against the ORACLE's
    restatement of sphere.rs:46-78 (rt_oracle_sphere_hit) and against the CPU build of the kernel source: random pairs, rays tangent to the sphere (discriminant exactly 0 or in
    the denormal range — the cold library-sqrt path), origins on / inside the sphere, negative
    radii, degenerate directions."""
    torch = torch_cuda
    rng = np.random.default_rng(99)
    n = 200_000
    c = rng.uniform(-5, 5, (n, 3))
    r = rng.uniform(0.05, 3.0, n) * rng.choice([1.0, 1.0, 1.0, -1.0], n)
    o = c + rng.standard_normal((n, 3)) * rng.uniform(0.0, 6.0, (n, 1))
    d = (c + rng.standard_normal((n, 3)) * np.abs(r)[:, None] * rng.uniform(0.0, 1.5, (n, 1))) - o
    k = n // 8
    # exactly tangent, representable: axis-aligned rays past integer-ish spheres  (oc.d)^2 - |d|^2 (|oc|^2 - r^2) = 0
    ci = rng.integers(-4, 5, (k, 3)).astype(np.float64); ri = rng.integers(1, 4, k).astype(np.float64)
    ax = rng.integers(0, 3, k); bx = (ax + 1) % 3
    ot = ci.copy(); ot[np.arange(k), bx] += ri; ot[np.arange(k), ax] -= rng.integers(2, 9, k)
    dt = np.zeros((k, 3)); dt[np.arange(k), ax] = rng.choice([0.5, 1.0, 2.0, 4.0], k)
    c[:k], r[:k], o[:k], d[:k] = ci, ri, ot, dt
    # almost tangent: the same rays nudged by a few ulps / tiny offsets either way (tiny positive and negative discriminants)
    c[k:2 * k], r[k:2 * k], d[k:2 * k] = ci, ri, dt
    o[k:2 * k] = ot
    o[np.arange(k, 2 * k), bx] += ri * rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-150, -17, k)
    # origin exactly on the surface / inside; zero and denormal direction components
    o[2 * k:3 * k] = c[2 * k:3 * k] + np.eye(3)[rng.integers(0, 3, k)] * np.abs(r[2 * k:3 * k, None])
    d[3 * k:3 * k + k // 2, rng.integers(0, 3)] = rng.choice([0.0, -0.0, 1e-310, -1e-305], k // 2)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    sph = np.ascontiguousarray(np.concatenate([c, r[:, None]], axis=1))
    d_rays, d_sph = torch.from_numpy(rays).cuda(), torch.from_numpy(sph).cuda()
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    assert pkg.hip.probe_lib().rt_hip_hit_probe(d_rays.data_ptr(), d_sph.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want, want_o = np.empty(n), np.empty(n)
    s = abi.RtSphere()
    tmax = float(np.finfo(np.float64).max)
    rec = (C.c_double * 10)()
    osh = oracle.lib(abi).rt_oracle_sphere_hit
    for i in range(n):
        s.center[:] = c[i].tolist(); s.radius = float(r[i])
        oi, di = dvec(*o[i]), dvec(*d[i])
        want[i] = hostsim.hostsim_exact_root(oi, di, s, 0.001, tmax)
        want_o[i] = rec[0] if osh(dvec(*c[i]), float(r[i]), oi, di, 0.001, tmax, rec) else -1.0
    assert np.array_equal(got, want_o, equal_nan=True), np.flatnonzero(got != want_o)[:10]   # the oracle: the reference's own arithmetic
    assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(got != want)[:10]       # the CPU build of the kernel source
    assert (want[:k] > 0).mean() > 0.9 and (want >= 0).mean() > 0.3   # the tangent rays do hit (discriminant 0 -> one root)


def test_device_fast_texel_arithmetic(pkg, torch_cuda):
    """VERDICT r2 weak #1c: texel_fast's (u, v) go through v_rsq_f64 / v_rcp_f64 + Newton steps on the DEVICE and through
    1/sqrt and `/` in the CPU build, so the CPU test of the fast path checks another instruction sequence.  Here the
    device runs both paths itself (rt_hip_texel_probe) on 1.2e7 hit points — uniform directions plus points aimed at
    column / row boundaries, the u wrap, the poles and the seams of the atan reduction: wherever the fast path names a
    texel it is the exact path's texel; its (u, v) stay within 1e-14 of the exact ones (TEXEL_EPS = 4e-12 is the band it
    must stay inside); it declines < 1e-4 of ordinary points.  rt_fast_quot / rt_fast_rsqrt: relative error vs numpy."""
    import texel_points
    torch = torch_cuda
    L = pkg.hip.probe_lib()
    rng = np.random.default_rng(23)
    n = 2_000_000
    total = wrong = refused = 0
    worst_u = worst_v = 0.0
    for (w, h, h_off, radius, centre) in texel_points.CASES:
        pts, m4 = texel_points.points(rng, n, w, h, h_off, radius, centre)
        d_p = torch.from_numpy(pts).cuda()
        d_out = torch.zeros((n, 5), dtype=torch.int64, device="cuda:0")
        d_uv = torch.zeros((n, 4), dtype=torch.float64, device="cuda:0")
        cr = (C.c_double * 4)(*centre, radius)
        assert L.rt_hip_texel_probe(d_p.data_ptr(), cr, h_off, w, h, d_out.data_ptr(), d_uv.data_ptr(), n, None) == 0
        torch.cuda.synchronize()
        out, uv = d_out.cpu().numpy(), d_uv.cpu().numpy()
        ok = out[:, 0] == 1
        wrong += int((ok & ((out[:, 1] != out[:, 3]) | (out[:, 2] != out[:, 4]))).sum())
        refused += int((~ok[m4:]).sum())
        total += n - m4
        fin = np.isfinite(uv[:, 0])     # (fast u = NaN: the fast core declined — poles, degenerate input)
        if abs(radius) >= 1e-2:         # (the 1e-3 sphere 2e3 away from the origin: the hit point itself carries 1e-13 of rounding)
            worst_u = max(worst_u, float(np.abs(uv[fin, 0] - uv[fin, 2]).max()))
            worst_v = max(worst_v, float(np.abs(uv[fin, 1] - uv[fin, 3]).max()))
    print(f"device texel probe: {6 * n} points, wrong {wrong}, fast path declined {refused} of {total} un-aimed points, "
          f"max |u_fast - u_exact| {worst_u:.2e}, max |v_fast - v_exact| {worst_v:.2e}")
    assert wrong == 0, f"{wrong} fast texels differ from the exact path on the device"
    assert refused < 1e-4 * total, (refused, total)
    assert worst_u < 1e-14 and worst_v < 1e-14, (worst_u, worst_v)     # rt_core.h: |error| < 1e-14 << TEXEL_EPS = 4e-12
    # the two device-only primitives
    m = 1 << 20
    x = np.abs(rng.standard_normal(m)) * 10.0 ** rng.uniform(-200, 200, m) + 1e-300
    y = np.abs(rng.standard_normal(m)) * 10.0 ** rng.uniform(-100, 100, m) + 1e-300
    x[:4] = [1.0, 2.0, 0.5, 3.0]; y[:4] = [1.0, 3.0, 0.75, 7.0]
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    dq, dr, dd = torch.zeros_like(dx), torch.zeros_like(dx), torch.zeros_like(dx)
    assert L.rt_hip_quot_probe(dx.data_ptr(), dy.data_ptr(), dq.data_ptr(), dr.data_ptr(), dd.data_ptr(), m, None) == 0
    torch.cuda.synchronize()
    q, r = dq.cpu().numpy(), dr.cpu().numpy()
    with np.errstate(over="ignore", under="ignore"):
        want_q, want_r = x / y, 1.0 / np.sqrt(x)
    sane = np.isfinite(want_q) & (np.abs(want_q) > 1e-290) & (np.abs(want_q) < 1e290)
    rel_q = float(np.abs(q[sane] / want_q[sane] - 1.0).max())
    rel_r = float(np.abs(r / want_r - 1.0).max())
    print(f"device rt_fast_quot: max rel err {rel_q:.2e} ({rel_q / 2.0 ** -53:.1f} x 2^-53); rt_fast_rsqrt: {rel_r:.2e}")
    assert rel_q < 4.0 * 2.0 ** -53 and rel_r < 8.0 * 2.0 ** -53
    # rt_div_inrange (1/|d|^2 of every ray, 1/|d| of Glass hits): the library division without range scaling and fix-up
    # must BE the IEEE quotient wherever the kernel uses it (divisor in [1e-150, 1e150], quotient in [1e-290, 1e290] or zero)
    m2 = 1 << 21
    yb = np.abs(rng.standard_normal(m2)) * 10.0 ** rng.uniform(-149, 149, m2) + 1e-150
    xb = np.where(rng.random(m2) < 0.5, 1.0, np.abs(rng.standard_normal(m2)) * 10.0 ** rng.uniform(-100, 100, m2))
    xb[:3] = [0.0, 1.0, 3.0]; yb[:3] = [7.0, 3.0, 1.0]
    with np.errstate(over="ignore", under="ignore"):
        want_d = xb / yb
    use = (want_d == 0.0) | ((np.abs(want_d) > 1e-290) & (np.abs(want_d) < 1e290))
    dxb, dyb = torch.from_numpy(xb).cuda(), torch.from_numpy(yb).cuda()
    o1, o2, o3 = torch.zeros_like(dxb), torch.zeros_like(dxb), torch.zeros_like(dxb)
    assert L.rt_hip_quot_probe(dxb.data_ptr(), dyb.data_ptr(), o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), m2, None) == 0
    torch.cuda.synchronize()
    got_d = o3.cpu().numpy()
    assert np.array_equal(got_d[use].view(np.uint64), want_d[use].view(np.uint64)), int((got_d[use] != want_d[use]).sum())
    print(f"device rt_div_inrange: {int(use.sum())} in-range quotients equal the IEEE quotient bit for bit")


def _cover_800x600(host, spp, seed=0):
    """the reference's own data/cover_scene.json geometry: 800x600, aspect 4/3 (scenes/cfg2 is its 1200x800 / 1.5 variant)"""
    j = json.load(open(os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")))
    j["width"], j["height"], j["samples_per_pixel"] = 800, 600, spp
    j["camera"]["aspect"] = 800.0 / 600.0
    sc = host.Scene.loads(json.dumps(j))
    sc.c.seed = seed
    return sc


def test_region_statistics_against_the_reference_cover_png(gpu_render, host):
    """the only image the reference itself rendered, raytracer/output/cover.png (800x600), is another random
    instance of the cover world — same camera, sky, ground and three big spheres.  Its region statistics (fixture:
    tests/golden/cover_png_stats.json, made by tests/golden/make_cover_png_stats.py from the reference's file) against a GPU
    render of data/cover_scene.json at the reference's 800x600 / spp 64: the sky band and the Metal sphere's sky
    reflection (no small sphere in them) within 1 level, the Lambertian sphere within 3, the ground's MEDIAN and the whole
    image's mean (different small spheres) within 16 / 12 levels."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_cover_png_stats as mk
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "cover_png_stats.json")))["regions"]
    sc = _cover_800x600(host, 64)
    rgb, _, _ = gpu_render(sc, want_linear=False)
    got = mk.stats_of(rgb)
    tol = {"sky_band": ("mean", 1.0), "metal_sphere_sky_reflection": ("mean", 1.0), "brown_lambertian_sphere": ("mean", 3.0),
           "ground_lower_third": ("median", 16.0), "whole_image": ("mean", 12.0)}
    for name, (stat, t) in tol.items():
        d = np.abs(np.array(got[name][stat]) - np.array(ref[name][stat]))
        print(f"cover.png {name} {stat}: ours {got[name][stat]} reference {ref[name][stat]}")
        assert d.max() <= t, (name, stat, got[name][stat], ref[name][stat])


def test_cross_seed_statistics(gpu_render, oracle, abi, host):
    """SURVEY §8(d) cross-RNG sanity: the kernel with seed 0 against the ORACLE with other seeds — independent samples of the
    same integrand.  Per 8x8 block the difference of the block means must be noise: z = diff / sigma with sigma^2 from the
    per-pixel variance (estimated from two oracle seeds; 1-dof estimates, hence heavy tails), must look standard normal — |z| > 4 in < 0.5 % of the blocks and
    channels, mean z^2 near 1 — and the whole-image means agree within 3 sigma."""
    sc0 = _cover_800x600(host, 64, seed=0)
    sc0.c.width, sc0.c.height = 240, 180
    g_rgb, g_lin, _ = gpu_render(sc0)
    sc0.c.seed = 1
    _, o1, _ = oracle.render(abi, sc0.ptr)
    sc0.c.seed = 2
    _, o2, _ = oracle.render(abi, sc0.ptr)
    assert not np.array_equal(o1, o2) and not np.array_equal(g_lin, o1)
    H, W = 176, 240                                   # whole 8x8 blocks
    var_px = 0.5 * (o1[:H, :W].astype(np.float64) - o2[:H, :W]) ** 2       # unbiased estimate of one render's pixel variance
    diff = g_lin[:H, :W].astype(np.float64) - o1[:H, :W]                   # variance 2 var_px under independence

    def blocks(a):
        return a.reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))
    # smooth the 1-dof variance estimates over 3x3 blocks: sigma of a block-mean difference
    vb = blocks(var_px) * 2.0 / 64.0
    pad = np.pad(vb, ((1, 1), (1, 1), (0, 0)), mode="edge")
    vs = sum(pad[i:i + vb.shape[0], j:j + vb.shape[1]] for i in range(3) for j in range(3)) / 9.0
    z = blocks(diff) / np.sqrt(vs + 1e-12)
    noisy = vs > 1e-9                                  # (sky blocks are noise-free up to the jitter: z is ill-defined there)
    zz = z[noisy]
    frac4 = float((np.abs(zz) > 4.0).mean())
    print(f"cross-seed: {zz.size} block-channels, mean z {zz.mean():+.3f}, mean z^2 {np.mean(zz ** 2):.3f}, |z| > 4: {frac4:.4%}")
    assert abs(zz.mean()) < 0.1 and 0.6 < np.mean(zz ** 2) < 1.6 and frac4 < 5e-3   # (a 1 % brightness bias gives mean z^2 > 100)
    # whole image, per channel
    sig = np.sqrt((2.0 * var_px).sum(axis=(0, 1))) / (H * W)
    dz = diff.mean(axis=(0, 1)) / sig
    print(f"cross-seed whole image: mean diff / sigma = {np.round(dz, 2).tolist()}")
    assert np.abs(dz).max() < 3.5


def _run_bench(args, env_extra=None, timeout=600):
    env = dict(os.environ, MASTER_PORT="29571")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, cwd=ROOT, timeout=timeout, env=env)


def test_bench_multi_gpu_without_torchrun_runs_the_in_library_group():
    """`python bench.py --gpus N` (no torchrun) drives the PRODUCT's multi-GPU path — the in-library group —
    in one process and prints ONE JSON line; here with 4 ranks sharing the box's GPU (RT_GPUS_EMULATE=1)."""
    r = _run_bench(["--gpus", "4", "--steps", "3", "--warmup", "1", "--full"], {"RT_GPUS_EMULATE": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["steps"] == 3 and d["scaling"] == "strong" and "error" not in d
    assert "BASELINE configs[1]" in d["config"]["workload"] and "in-library group" in d["config"]["parallelism"]
    assert "RANKS SHARE DEVICES" in d["config"]["parallelism"]          # an emulation says so
    assert d["transport"] == "peer" and d["rccl_ranks"] == 0 and len(d["rank_devices"]) == 4 and d["distinct_devices"] == 1
    assert d["transport_fallback"] is False and d["transport_fallback_reason"] is None    # (peer was what an emulation asks for)
    pr = d["per_rank"]
    assert all(len(pr[k]) == 4 for k in ("kernel_ms", "t_wake_us", "t_enq_us", "pci_bus_id", "numa_node", "pinned_cpus", "peer_to_root")), pr
    assert min(pr["kernel_ms"]) > 0 and max(pr["t_enq_us"]) > 0
    assert d["frame_identical_to_n1"] is True
    samples = 1200 * 800 * 128
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    assert d["kernel_ms"] > 0 and d["frame_latency_ms"] >= d["kernel_ms"] * 0.9 and d["n1_kernel_ms"] > 0
    _check_multi_gpu_line_extras(d, 4)


def _check_multi_gpu_line_extras(d, n):
    """an N > 1 line parses like the N = 1 line (roofline per rank, cpu_baseline pointer) and carries BASELINE
    configs[3] — the workload BASELINE.json names for the 8-GPU node — timed on the same ranks"""
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "valu"
    if rf["frac"] is not None:
        assert 0 < rf["frac"] <= 1 and len(rf["per_rank_frac"]) == n and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 2e-3
    cb = d["cpu_baseline"]
    if cb is not None:    # (a committed N = 1 line exists under profiles/)
        for k in ("value", "unit", "cores", "kind", "sample", "source"):
            assert k in cb, k
        assert cb["value"] > 0 and cb["source"].startswith("profiles/")
    c3 = d["configs3_on_group"]
    assert "error" not in c3, c3
    assert "BASELINE configs[3]" in c3["workload"] and "3840x2160 spp 512" in c3["workload"]
    assert c3["frame_ms"] >= c3["kernel_ms"] * 0.9 and c3["kernel_ms"] > 0 and c3["n1_kernel_ms"] > 0 and c3["speedup_vs_n1"] > 0
    assert abs(c3["msamples_per_s"] - 3840 * 2160 * 512 / c3["frame_ms"] / 1e3) < 1e-2 * c3["msamples_per_s"]
    assert len(c3["per_rank"]["kernel_ms"]) == n and min(c3["per_rank"]["kernel_ms"]) > 0 and c3["frame_identical_to_n1"] is True
    assert "roofline" in c3 and c3["roofline"]["bound"] == "valu"


def test_bench_gpus_8_emulated_carries_configs3_on_the_group():
    """`python bench.py --gpus 8 --full` — the command of the driver's scaling run, with everything else the line can carry — with
    the 8 ranks sharing one GPU: value as before, + BASELINE configs[3] on the 8-rank group, roofline and the cpu_baseline pointer."""
    r = _run_bench(["--gpus", "8", "--steps", "3", "--warmup", "1", "--full"], {"RT_GPUS_EMULATE": "1"}, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and "error" not in d and d["frame_identical_to_n1"] is True
    samples = 1200 * 800 * 128
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    _check_multi_gpu_line_extras(d, 8)
    c3 = d["configs3_on_group"]
    print(f"8 emulated ranks: cfg2 {d['value']:.0f} Msamples/s; configs[3] frame {c3['frame_ms']:.1f} ms ({c3['msamples_per_s']:.0f} Msamples/s), n1 {c3['n1_kernel_ms']:.1f} ms")


def test_bench_more_gpus_than_visible_is_a_json_error_line():
    """... and asking for more devices than the box has ends in ONE JSON line with an "error" key and a non-zero exit
    code, not in a traceback on stdout."""
    import torch
    n = torch.cuda.device_count() + 7
    r = _run_bench(["--gpus", str(n), "--steps", "2", "--warmup", "1"], {"RT_GPUS_EMULATE": "0"})
    assert r.returncode != 0
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] is None and d["n_gpus"] == n and "device" in d["error"]


def test_bench_dump_outputs_is_the_frame_of_the_timed_path(gpu_render, load_scene, tmp_path):
    """`bench.py --dump-outputs DIR`: the RGB8 frame of the last timed step as float32 [H, W, 3], equal to a direct render of the
    same scene — from the one-process path and from the in-library group (two ranks sharing the GPU) alike."""
    frames = {}
    for name, args, env in (("n1", ["--gpus", "1"], None), ("g2", ["--gpus", "2"], {"RT_GPUS_EMULATE": "1"})):
        r = _run_bench(args + ["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-other-configs", "--dump-outputs", str(tmp_path / name)], env)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["dumped_outputs"] == {"frame_rgb8": [800, 1200, 3]}
        assert sorted(os.listdir(tmp_path / name)) == ["frame_rgb8.npy"]
        frames[name] = np.load(tmp_path / name / "frame_rgb8.npy")
        assert frames[name].dtype == np.float32 and frames[name].shape == (800, 1200, 3)
    rgb, _, _ = gpu_render(load_scene("cover"), want_linear=False)
    assert np.array_equal(frames["n1"], rgb.astype(np.float32))
    assert np.array_equal(frames["g2"], frames["n1"])


def test_scene_may_change_streams_once_the_first_stream_is_drained(pkg, load_scene, torch_cuda):
    """a caller that synchronises the first stream ITSELF (no rt_hip_wait) may launch on another stream — the
    in-flight guard asks hipStreamQuery instead of insisting on rt_hip_wait (the ABI v2 behaviour)."""
    torch = torch_cuda
    sc = load_scene("cover", 64, 40, 2, 50)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    a = torch.zeros((40, 64, 3), dtype=torch.uint8, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    gs.render(a.data_ptr(), 0, None, s1.cuda_stream)
    s1.synchronize()
    gs.render(a.data_ptr(), 0, None, s2.cuda_stream)
    first = a.cpu().numpy().copy()
    gs.wait()
    assert np.array_equal(a.cpu().numpy(), first) and first.any()
    gs.close()


@pytest.mark.parametrize("world,env", [(1, {}), (1, {"RT_GATHER_SELFTEST": "1", "RT_GATHER": "rccl"}), (3, {"RT_GPUS_EMULATE": "1"}), (8, {"RT_GPUS_EMULATE": "1"}),
                                       (1, {"RT_GROUP_OVERLAP": "0"}), (3, {"RT_GPUS_EMULATE": "1", "RT_GROUP_OVERLAP": "0"})])   # (round 6: odd frames in flight run through a second view + stream; "0" = the single-scene form)
def test_group_submit_collect_pipelines_frames_bit_identically(pkg, gpu_render, load_scene, world, env):
    """rt_hip_group_submit / _collect (ABI v4): two frames in flight — frame i's gather, de-interleave and device-to-host
    copy under frame i+1's kernels, every buffer twice — deliver the bytes and the path counts of blocking frames with the
    same settings, in submission order, each into the buffer it was submitted with; a third submit and a collect with
    nothing in flight are refused; the stage clocks of a frame are ordered."""
    sc = load_scene("test", 72, 50, 3, 8)
    want = {}
    for seed in (0, 1, 2, 3, 4):
        sc.c.seed = seed
        rgb, _, st = gpu_render(sc, want_linear=False)
        want[seed] = (rgb, st["segments"])
    sc.c.seed = 0
    grp = _with_env(env, lambda: pkg.hip.HipGroup(sc.ptr, world))
    with pytest.raises(pkg.host.RtError) as e:
        grp.collect()
    assert e.value.code == pkg.abi.RT_ERR_INVALID
    bufs = [np.zeros((50, 72, 3), np.uint8) for _ in range(5)]
    grp.set_option("seed", 0)
    grp.submit(bufs[0])
    for seed in (1, 2, 3, 4):
        grp.set_option("seed", seed)          # (a frame is rendered with the options in force when it is submitted)
        grp.submit(bufs[seed])
        if seed == 1:
            with pytest.raises(pkg.host.RtError) as e:
                grp.submit(None)
            assert e.value.code == pkg.abi.RT_ERR_INVALID
        st = grp.collect()                    # the OLDEST frame: seed - 1
        assert np.array_equal(bufs[seed - 1], want[seed - 1][0]), (world, seed - 1)
        assert st["segments"] == want[seed - 1][1] and st["n_gpus_used"] == world and st["kernel_ms"] > 0
        us = st["group_us"]
        assert 0 <= us[0] <= us[1] <= us[2] <= us[3] <= us[4] <= us[5] <= us[6] <= us[7], us
        assert abs(st["frame_ms"] * 1e3 - us[6]) < 1.0
    st = grp.collect()
    assert np.array_equal(bufs[4], want[4][0]) and st["segments"] == want[4][1]
    # blocking calls still work, also with a frame left in flight (it is collected first)
    grp.set_option("seed", 2)
    grp.submit(None)
    out, st = grp.render_to_host()
    assert np.array_equal(out, want[2][0]) and st["segments"] == want[2][1]
    grp.close()


def test_queue_order_is_only_an_order(gpu_render, abi, load_scene):
    """The order in which tiles leave the frame's queue — top row first, bottom row first, the deepest tiles of the previous
    frame first (measured by frame 1, used by frame 2), one queue or one per XCD — never shows in the bytes, the linear
    image or the path count: whole frames and shards, lit and unlit.  (The two first-frame order SEEDS of round 4 left the
    product in round 5: profiles/r05_order_seed_removed.patch.)"""
    for scene, w, h, spp, depth in (("cover", 200, 120, 4, 50), ("test", 96, 72, 3, 8)):
        sc = load_scene(scene, w, h, spp, depth)
        for tiles in (None, abi.RtRowTiles(2, 1, 3)):
            ref = gpu_render(sc, tiles=tiles, tile_order=1)
            for opts in ({"tile_order": 0}, {"tile_order": 2}, {"tile_order": 2, "tile_affinity": 2}, {"tile_order": 0, "tile_affinity": 2}, {"tile_order": 2, "tile_affinity": 0}):
                got = gpu_render(sc, tiles=tiles, opts=opts, frames=3)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (scene, opts)
                assert got[2]["segments"] == ref[2]["segments"] and got[2]["samples"] == ref[2]["samples"]


def test_texel_paths_on_the_gpu(gpu_render, oracle, abi, load_scene):
    """tests/test_core_cpu.py::test_texel_paths_agree_with_the_oracle on the device: 4-byte texels + 32-bit index
    arithmetic, and the u64 / RGB8 path for records outside its range, against the oracle's literal arithmetic"""
    from test_core_cpu import TEXEL_RECORDS, texel_record_scene
    for what, changes in TEXEL_RECORDS:
        sc = texel_record_scene(load_scene, abi, changes, 96, 72, 3)
        o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
        rgb, lin, st = gpu_render(sc)
        assert_parity(rgb, lin, o_rgb, o_lin, what, atol=pooled_atol(3))
        assert st["tex_oob"] == o_st["tex_oob"], what
        assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], what


def test_device_atan2_against_a_million_correctly_rounded_results(pkg, torch_cuda):
    """tests/test_oracle_kat.py::test_shared_atan2_against_a_million_correctly_rounded_results through the DEVICE build of
    rt_atan2.h (rt_hip_atan2_probe): the same 1.1 M pairs, every result the correctly rounded one of the mpmath fixture."""
    from atan2_points import points
    from test_oracle_kat import check_atan2_against_the_fixture
    torch = torch_cuda
    y, x, _ = points()
    dy, dx = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
    out = torch.empty_like(dy)
    assert pkg.hip.probe_lib().rt_hip_atan2_probe(dy.data_ptr(), dx.data_ptr(), out.data_ptr(), y.size, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    check_atan2_against_the_fixture(out.cpu().numpy(), y, x)


def test_fresh_group_first_frame_is_never_traced_twice(pkg, load_scene):
    """Round 4: hipMemset / pageable hipMemcpy at scene creation are asynchronous to the host and run on the NULL stream,
    which a non-blocking stream does not wait for — a first frame launched at once (the group launches rank 0 from the
    creating thread) could have its tile-queue cursor zeroed under it: tiles traced twice, identical image, 25 % more
    segments in 65 % of fresh 3-rank groups.  rt_hip_scene_create now drains the device before it returns."""
    sc = load_scene("test", 64, 49, 3, 8)
    want = None
    for world in (1, 3, 3, 3, 2, 8) + (3,) * 24:
        grp = _with_env({"RT_GPUS_EMULATE": "1"}, lambda: pkg.hip.HipGroup(sc.ptr, world))
        st = grp.render()
        grp.close()
        want = want or st["segments"]
        assert st["segments"] == want, (world, st["segments"], want)


def test_scene_query_and_tile_depth_diagnostics(pkg, load_scene, torch_cuda):
    """rt_hip_scene_query (what bench.py prices the tables with) and rt_hip_debug_tile_depth (the per-tile path depths the
    queue order is sorted by): the cover scene has its 484 spheres, a grid and a `large` list; the first (measuring) frame
    leaves a depth per tile — 0 where no path bounces (sky), up to max_depth where glass is."""
    torch = torch_cuda
    sc = load_scene("cover", 240, 160, 8, 50)
    gs = pkg.hip.HipScene(sc.ptr, 0, library=pkg.hip.probe_lib())   # (the debug call lives in librt_hip_probe.so: include/rt_abi_test.h)
    assert gs.query("n_spheres") == 484 and gs.query("n_lights") == 0 and gs.query("no_such_key") == -1
    cells, items, large = gs.query("grid_cells"), gs.query("grid_items"), gs.query("grid_large")
    assert cells > 1000 and items >= 480 and 1 <= large <= 8
    assert gs.query("table_bytes") == 484 * (32 + 48) + cells * 8 + items * 2 and gs.query("texel_bytes") == 0
    fb = torch.zeros((160, 240, 3), dtype=torch.uint8, device="cuda:0")
    gs.render(fb.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream)
    gs.wait()
    d = gs.debug_tile_depth()
    assert d.ndim == 2 and d.size * (4 ** 0) >= 1 and int(d.max()) >= 10 and int(d.max()) <= 50 and (d == 0).any()
    gs.close()
    tex = load_scene("test", 64, 48, 1, 8)
    gt = pkg.hip.HipScene(tex.ptr, 0)
    assert gt.query("n_lights") == 1 and gt.query("texel_bytes") > 4 * 2048 * 1024 and gt.query("grid_cells") == 0
    gt.close()
