"""Lens and motion frames at full size and through the whole machinery of the persistent kernel, against the C oracle's lens and
shutter (oracle/rt_oracle.h RtOracleExt, pinned on the CPU by tests/test_oracle_lens_motion.py).

The bar is the static full-size tests' (tests/test_gpu_parity.py): whole frames `atol=pooled_atol(spp), flip_frac=5e-4`, single
scanlines `flip_frac=2e-3`, and the path count `segments == oracle segments - segments_discarded` exactly, lit scenes included.
Whole frames of the two shipped 1200 x 800 scenes are compared at spp 32 — samples are addressed by (pixel, s), so that is the first
quarter of the shipped 128-spp frame — and 16 whole scanlines of each at the full 128 spp; no pixel, row or case is masked out.
Every whole-frame check prints size, spp, worst |dlin|, RGB8 flips, the segments of both sides and the oracle's wall time."""
import json
import os
import sys
import time

import numpy as np
import pytest

import ext_scenes as X
from ext_scenes import LDS, LENS, MOTION
from fuzz_worlds import big_flat_world_json, fuzz_world_json
from parity import assert_parity, pooled_atol
from test_motion import _every_other, _moving_cfg, _textured

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(X.ROOT, "scenes"))
WIDE = 8
# scanlines of the 1200 x 800 cover view: row 0, sky, the horizon and the first small spheres (60, 100), the three big spheres (200 -
# 450), the small spheres in front of them, which cover the ground down to the last row
COVER_ROWS = (0, 30, 60, 100, 200, 250, 300, 350, 400, 450, 500, 550, 625, 700, 775, 799)
MOVER_ROWS = tuple(y for y in COVER_ROWS if y >= 100)    # the rows that look at bouncing spheres


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def gpu(pkg, abi, torch_cuda):
    torch = torch_cuda

    def _render(sc, center1=None, lens=None, spp=None, tiles=None, frames=1, opts=None, library=None, query=None):
        """a fresh resident scene (moving if center1, through the lens if lens) -> (rgb8, linear, stats, last_kernel)"""
        gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=center1)
        if lens is not None:
            gs.set_lens(*lens)
        if spp is not None:
            gs.set_option("samples_per_pixel", spp)
        for k, v in (opts or {}).items():
            gs.set_option(k, v)
        rows = abi.tiles_local_rows(sc.c.height, tiles)
        rgb = torch.zeros((rows, sc.c.width, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((rows, sc.c.width, 3), dtype=torch.float32, device="cuda:0")
        for _ in range(frames):   # (frames > 1: the later frames use the queue order learnt from the one before)
            gs.render(rgb.data_ptr(), lin.data_ptr(), tiles, torch.cuda.current_stream().cuda_stream)
            st = gs.wait()
        if query is not None:
            query.update({k: gs.query(k) for k in ("motion", "lens", "lds_tables", "table_bytes", "grid_wide", "grid_large", "n_lights")})
        out = rgb.cpu().numpy(), lin.cpu().numpy(), st, gs.query("last_kernel")
        gs.close()
        return out
    return _render


def _whole_frame(oracle, abi, sc, got, spp, what, **ext):
    """a whole GPU frame against the oracle's at `spp`: the bar, the exact path count, and the line the issue asks for"""
    rgb, lin, st, _ = got
    sc.c.samples_per_pixel = spp
    t0 = time.time()
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr, **ext)
    wall = time.time() - t0
    d = np.abs(lin.astype(np.float64) - o_lin.astype(np.float64))
    flips = int((rgb != o_rgb).sum())
    print(f"{what}: WHOLE frame {sc.c.width} x {sc.c.height}, spp {spp} ({st['samples'] / 1e6:.2f} M samples) vs oracle: max |dlin| {d.max():.2e}, "
          f"rgb8 flips {flips} of {rgb.size}, segments gpu {st['segments']} oracle {o_st['segments']} - {o_st['segments_discarded']} discarded, "
          f"oracle {wall:.1f} s on {oracle.lib(abi).rt_oracle_threads()} threads, kernel {st['kernel_ms']:.2f} ms")
    assert st["samples"] == o_st["samples"] == sc.c.width * sc.c.height * spp
    assert_parity(rgb, lin, o_rgb, o_lin, what, atol=pooled_atol(spp), flip_frac=5e-4)
    assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (what, st["segments"], o_st["segments"], o_st["segments_discarded"])
    assert st["tex_oob"] == o_st["tex_oob"], (what, st["tex_oob"], o_st["tex_oob"])
    return o_rgb, o_lin, o_st


def _rows(oracle, abi, sc, got, rows, spp, what, x_range=None, **ext):
    """whole scanlines (or windows of them) of a GPU frame against the oracle at `spp` -> (worst |dlin|, {row: oracle linear})"""
    rgb, lin, _, _ = got
    sc.c.samples_per_pixel = spp
    x0, x1 = x_range or (0, sc.c.width)
    worst, seen = 0.0, {}
    for y in rows:
        o_rgb, o_lin, _ = oracle.render(abi, sc.ptr, abi.RtRowTiles(1, y, 1 << 20), x_range=x_range, **ext)
        err, _ = assert_parity(rgb[y:y + 1, x0:x1], lin[y:y + 1, x0:x1], o_rgb[:, x0:x1], o_lin[:, x0:x1], f"{what} row {y}",
                               atol=pooled_atol(spp), flip_frac=2e-3)
        worst = max(worst, err)
        seen[y] = o_lin[0, x0:x1]
    return worst, seen


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: frames differ"
    assert a[2]["segments"] == b[2]["segments"], (what, a[2]["segments"], b[2]["segments"])


def _full_size_programme(gpu, oracle, abi, sc, what, bits, **ext):
    """the headline test's programme (test_full_size_headline_config_properties) for a 1200 x 800 cover scene with an extension"""
    c = sc.c
    assert (c.width, c.height, c.samples_per_pixel, c.max_depth, c.n_spheres) == (1200, 800, 128, 50, 484)
    q = {}
    full = gpu(sc, query=q, **ext)
    assert full[3] & (LENS | MOTION) == bits and full[3] & LDS and q["lds_tables"] == 1, (what, full[3], q)
    assert full[2]["samples"] == 1200 * 800 * 128 and 2.0 < full[2]["segments"] / full[2]["samples"] < 3.5
    _same(gpu(sc, **ext), full, f"{what}: a second render")
    # three frames through the per-XCD queues: the third runs in the queue order learnt from the ones before
    _same(gpu(sc, frames=3, opts={"tile_affinity": 1}, **ext), full, f"{what}: three frames, tile_affinity 1")
    _same(gpu(sc, opts={"tile_affinity": 0, "tile_log2": 3}, **ext), full, f"{what}: one queue, 8 x 8 tiles")
    # shard invariance: rank 3 of 8 renders exactly its scanlines of the frame
    t = abi.RtRowTiles(8, 3, 8)
    rows = abi.tiles_global_rows(800, t)
    shard = gpu(sc, tiles=t, **ext)
    assert np.array_equal(shard[0], full[0][rows]) and np.array_equal(shard[1].view(np.uint32), full[1][rows].view(np.uint32)), what
    # 16 whole scanlines at the scene's own 128 spp
    worst, o_rows = _rows(oracle, abi, sc, full, COVER_ROWS, 128, what, **ext)
    print(f"{what}: {len(COVER_ROWS)} scanlines x 1200 px x 128 spp vs oracle, max |dlin| {worst:.2e}, kernel {full[2]['kernel_ms']:.2f} ms")
    # the whole frame at spp 32: the first quarter of the shipped frame's samples
    quarter = gpu(sc, spp=32, **ext)
    assert quarter[3] == full[3]
    _, o_lin, o_st = _whole_frame(oracle, abi, sc, quarter, 32, what, **ext)
    assert o_st["segments_discarded"] == 0
    c.samples_per_pixel = 128
    return full, o_rows, o_lin


def test_full_size_depth_of_field_scene(gpu, oracle, abi, host):
    """scenes/cover_dof_1200x800_spp128.json through rt_hip_set_lens at 1200 x 800: the LENS + LDS kernel, determinism, the learnt
    queue order, a row shard, 16 scanlines at 128 spp and the whole frame at spp 32 (30.7 M samples: ~1.4 M lens draws take a
    second Philox call, ~65 k a third; every lane refills thousands of times) against the oracle"""
    sc, c1, lens = X.load(host, X.DOF)
    assert c1 is None and lens[2] == 0.05
    full, o_rows, _ = _full_size_programme(gpu, oracle, abi, sc, "dof scene", LENS, lens=lens)
    # conditions on the oracle alone: the lens blurs the rows that hold geometry away from the focus plane
    for y in (300, 700):
        pin = oracle.render(abi, sc.ptr, abi.RtRowTiles(1, y, 1 << 20))[1][0]
        assert not np.array_equal(pin, o_rows[y]), y


def test_full_size_motion_blur_scene(gpu, oracle, abi, host):
    """scenes/cover_motion_1200x800_spp128.json through HipScene(center1=): 405 bouncing spheres, the MOTION + LDS kernel over the
    taller swept boxes, the same programme"""
    sc, c1, lens = X.load(host, X.MOTION_SCENE)
    assert lens is None and c1 is not None
    q = {}
    gpu(sc, center1=c1, spp=1, query=q)
    assert q["motion"] == 405
    full, o_rows, _ = _full_size_programme(gpu, oracle, abi, sc, "motion scene", MOTION, center1=c1)
    # conditions on the oracle alone: each row chosen for the small spheres really sees movers
    for y in MOVER_ROWS:
        still = oracle.render(abi, sc.ptr, abi.RtRowTiles(1, y, 1 << 20))[1][0]
        assert not np.array_equal(still, o_rows[y]), f"row {y}: the motion oracle's row is the static oracle's"


def test_full_size_lens_and_motion_together(gpu, oracle, abi, host):
    """the motion scene through the depth-of-field scene's camera: the LENS + MOTION kernel, whole frame at spp 32"""
    cfg = X.config(X.MOTION_SCENE)
    dof = X.config(X.DOF)["camera"]
    cfg["camera"].update(aperture=dof["aperture"], focus_dist=dof["focus_dist"])
    sc, c1, lens = X.load(host, cfg)
    assert c1 is not None and lens[2] == 0.05 and (sc.c.width, sc.c.height) == (1200, 800)
    ext = dict(center1=c1, lens=lens)
    got = gpu(sc, spp=32, **ext)
    assert got[3] & (LENS | MOTION) == LENS | MOTION and got[3] & LDS
    _same(gpu(sc, spp=32, frames=3, opts={"tile_affinity": 1}, **ext), got, "lens + motion: three frames, tile_affinity 1")
    _, o_lin, _ = _whole_frame(oracle, abi, sc, got, 32, "lens + motion", **ext)
    # on the oracle alone: neither extension is idle (two rows, against the frame with only the other one)
    for y in (300, 700):
        t = abi.RtRowTiles(1, y, 1 << 20)
        assert not np.array_equal(oracle.render(abi, sc.ptr, t, center1=c1)[1][0], o_lin[y])
        assert not np.array_equal(oracle.render(abi, sc.ptr, t, lens=lens)[1][0], o_lin[y])


def test_full_size_lit_scene_with_movers_and_a_lens(gpu, oracle, abi, host):
    """scenes/cfg1_test_800x600_spp16.json at 800 x 600, spp 16 (a Light, textures, sky texture, Metal, hollow Glass) with every
    other sphere moving and a lens: tau held across suspended light activations over a whole lit frame; the path count is the
    oracle's minus the light loops the reference discards, exactly"""
    cfg = _moving_cfg(X.TEST, np.random.default_rng(41), _every_other, {"aperture": 0.2, "focus_dist": 2.0})
    sc, c1, lens = X.load(host, cfg)
    c = sc.c
    assert (c.width, c.height, c.samples_per_pixel, c.max_depth) == (800, 600, 16, 8) and len(sc.lights()) == 1 and c1 is not None
    ext = dict(center1=c1, lens=lens)
    q = {}
    got = gpu(sc, query=q, **ext)
    assert got[3] & (LENS | MOTION) == LENS | MOTION and got[3] & 4 and q["motion"] >= 2 and q["n_lights"] == 1, (got[3], q)
    _same(gpu(sc, **ext), got, "lit: a second render")
    _, o_lin, o_st = _whole_frame(oracle, abi, sc, got, 16, "lit test scene, movers + lens", **ext)
    assert o_st["segments_discarded"] > 0 and got[2]["tex_oob"] == 0 == o_st["tex_oob"]
    still = oracle.render(abi, sc.ptr, abi.RtRowTiles(1, 300, 1 << 20), lens=lens)[1][0]
    assert not np.array_equal(still, o_lin[300])


def test_textured_4k_scene_with_movers(gpu, oracle, abi, host):
    """scenes/cfg3_cover_4k_textured.json at 3840 x 2160 with its textured spheres (and every third sphere) moving sideways: the
    texture's (u, v) from the centre at tau; whole frame on the GPU at spp 64, whole scanlines through the sky texture, the
    textured spheres and the ground against the oracle"""
    cfg = _moving_cfg(X.TEX, np.random.default_rng(43), _textured)
    sc, c1, lens = X.load(host, cfg, spp=64)
    c = sc.c
    assert (c.width, c.height, c.n_spheres) == (3840, 2160, 484) and c.sky_mode == abi.RT_SKY_TEXTURE and lens is None
    q = {}
    got = gpu(sc, center1=c1, query=q)
    assert got[3] & MOTION and not got[3] & (LENS | WIDE | 4) and bool(got[3] & LDS) == bool(q["lds_tables"]), (got[3], q)
    assert got[2]["tex_oob"] == 0 and got[2]["samples"] == 3840 * 2160 * 64
    rows = (40, 700, 900, 1080, 1300, 1500, 1900, 2159)
    worst, o_rows = _rows(oracle, abi, sc, got, rows, 64, "textured 4K with movers", center1=c1)
    print(f"textured 4K with movers: {len(rows)} scanlines x 3840 px x 64 spp vs oracle, max |dlin| {worst:.2e}, last_kernel {got[3]}, "
          f"tables in LDS {q['lds_tables']} ({q['table_bytes']} B)")
    for y in (900, 1080, 1300):   # (on the oracle alone: the rows through the textured spheres see them move)
        assert not np.array_equal(oracle.render(abi, sc.ptr, abi.RtRowTiles(1, y, 1 << 20))[1][0], o_rows[y]), y


def _flat_world_with_movers(host, n, seed, width, height, spp, lens_keys=None):
    """fuzz_worlds.big_flat_world_json with a third of its small spheres moving (sideways and up, by up to 2.5 radii)"""
    cfg = json.loads(big_flat_world_json(n, np.random.default_rng(seed), width=width, height=height, spp=spp))
    cfg["camera"].update(lens_keys or {})
    rng = np.random.default_rng(seed + 1)
    offs = rng.uniform((-0.5, 0.0, -0.5), (0.5, 0.5, 0.5), (n + 1, 3))
    for i, o in enumerate(cfg["objects"]):
        if i % 3 == 1:
            c = o["center"]
            o["center1"] = {"x": c["x"] + float(offs[i, 0]), "y": c["y"] + float(offs[i, 1]), "z": c["z"] + float(offs[i, 2])}
    return X.load(host, cfg)


def test_l2_tables_world_with_movers(gpu, oracle, abi, host):
    """6 000 spheres (tables above LDS_TABLES_MAX_BYTES: the kernel gathers them from L2), a third of them moving, with and without
    a lens: the whole 240 x 160 frame against the oracle's scan over all 6 001 spheres, and the full scan on the device bit for bit"""
    sc, c1, _ = _flat_world_with_movers(host, 6000, 11, 240, 160, 4)
    assert sc.c.n_spheres == 6001
    q = {}
    got = gpu(sc, center1=c1, query=q)
    assert got[3] & MOTION and not got[3] & (LDS | WIDE) and q["lds_tables"] == 0 and q["motion"] == 2000 and q["table_bytes"] > 156 * 1024, (got[3], q)
    assert got[2]["grid_steps"] > 0 and got[2]["exact_tests"] < got[2]["sphere_tests"]
    _whole_frame(oracle, abi, sc, got, 4, "L2 tables, 6 001 spheres, 2 000 movers", center1=c1)
    _same(gpu(sc, center1=c1, opts={"variant": 1}), got, "L2 tables: grid walk vs full scan")
    assert not np.array_equal(gpu(sc)[1], got[1])
    sc2, c2, lens = _flat_world_with_movers(host, 6000, 11, 240, 160, 4, {"aperture": 0.2, "focus_dist": 12.0})
    assert c2 == c1 and lens is not None
    both = gpu(sc2, center1=c1, lens=lens)
    assert both[3] & (LENS | MOTION) == LENS | MOTION and not both[3] & (LDS | WIDE)
    _whole_frame(oracle, abi, sc2, both, 4, "L2 tables, movers + lens", center1=c1, lens=lens)


def test_wide_tables_world_with_movers(gpu, oracle, abi, host):
    """66 001 spheres (32-bit item lists, the wide instantiations), 22 000 of them moving, at test_more_than_65535_spheres' size"""
    n = 66000
    sc, c1, _ = _flat_world_with_movers(host, n, 3, 24, 16, 2)
    assert sc.c.n_spheres == n + 1
    q = {}
    got = gpu(sc, center1=c1, query=q)
    assert got[3] & MOTION and got[3] & WIDE and not got[3] & LDS and q["grid_wide"] == 1 and q["motion"] == n // 3, (got[3], q)
    assert got[2]["grid_steps"] > 0 and got[2]["exact_tests"] < got[2]["sphere_tests"]
    _whole_frame(oracle, abi, sc, got, 2, "wide tables, 66 001 spheres, 22 000 movers", center1=c1)
    _same(gpu(sc, center1=c1, opts={"variant": 1}), got, "wide tables: grid walk vs full scan")
    assert not np.array_equal(gpu(sc)[1], got[1])


@pytest.mark.parametrize("with_lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("kind", range(6))
def test_fuzz_worlds_with_movers_grid_equals_full_scan_equals_oracle(gpu, oracle, abi, host, kind, with_lens):
    """the triangle of test_fuzz_worlds_grid_equals_bruteforce_on_the_gpu on MOVING worlds: tests/fuzz_worlds.py kinds 0 - 5 with
    three quarters of the non-light spheres moving (along an axis, diagonally, or across many cells, by kind), with and without a
    lens: the grid kernel against the oracle at the bar, against `variant` 1 (the full scan with every centre at the lane's tau)
    bit for bit with the same path count, and the frame is not the static world's"""
    rng = np.random.default_rng(3000 + kind)
    cfg = json.loads(fuzz_world_json(rng, kind))
    if with_lens:
        cfg["camera"].update(aperture=0.3, focus_dist=6.0)
    sc, none, lens = X.load(host, cfg)
    assert none is None and (lens is not None) == with_lens
    c1 = X.move_some(abi, sc, rng, ("axis", "diag", "long")[kind % 3])
    ext = dict(center1=c1.tolist(), lens=lens)
    what = f"moving fuzz world {kind}{' + lens' if with_lens else ''}"
    q = {}
    grid = gpu(sc, query=q, **ext)
    assert q["motion"] > 50 and grid[3] & MOTION and bool(grid[3] & LENS) == with_lens, (what, q, grid[3])
    _whole_frame(oracle, abi, sc, grid, sc.c.samples_per_pixel, what, **ext)
    scan = gpu(sc, opts={"variant": 1}, **ext)
    _same(scan, grid, f"{what}: grid walk vs full scan")
    assert scan[2]["exact_tests"] == scan[2]["sphere_tests"]
    if kind != 2:
        assert grid[2]["grid_steps"] > 0, "the world is expected to be gridded"
    assert not np.array_equal(gpu(sc, lens=lens)[1], grid[1]), f"{what}: the static world's frame"
