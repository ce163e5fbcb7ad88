"""Adaptive sampling (include/rt_abi.h rt_hip_tile_grid / rt_hip_accumulate_tiles / rt_hip_tile_error / rt_hip_resolve_tiles /
rt_hip_render_adaptive_to_host, the CLI's --adaptive): per-tile sample counts over the accumulating kernels' own
pixel tiles.

A tile holding samples [0, n_t) is, pixel for pixel, the one-shot frame at n_t samples BIT FOR BIT.  The noise estimate is a fixed
sequence of IEEE f64 operations, restated here in numpy and compared bit for bit; the schedule is replayed here from errors the test
computes itself."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from parity import LINEAR_ATOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_hip_tile_grid", "rt_hip_accumulate_tiles", "rt_hip_tile_error", "rt_hip_resolve_tiles", "rt_hip_render_adaptive_to_host")
F = np.uint64(1 << 63)   # sticky NaN flag of an accumulator word
GUARD = np.uint64(0x0123456789ABCDEF)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _cli(args, env=None):
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    return subprocess.run([exe, *args], capture_output=True, text=True, cwd=ROOT, timeout=120, env=env)


# ---------------------------------------------------------------------------------------------------- numpy restatements

def np_tile_error(now, prev, n_now, n_prev, grid, rows, width):
    """DESIGN.md §11's estimate, operation for operation: per-tile max of e over the pixels without a NaN flag ([tiles_y, tiles_x])"""
    tw, th, tx, ty = grid
    P = prev.reshape(rows, width, 3).view(np.uint64)
    Q = now.reshape(rows, width, 3).view(np.uint64)
    ok = ~(((P | Q) & F) != 0).any(axis=2)
    sa = np.float64(n_prev) * np.float64(2.0 ** 40)
    sb = np.float64(n_now - n_prev) * np.float64(2.0 ** 40)
    with np.errstate(all="ignore"):
        a = P.astype(np.float64) / sa
        b = (Q - P).astype(np.float64) / sb
        d = (np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])) + np.abs(a[..., 2] - b[..., 2])
        s = ((a[..., 0] + b[..., 0]) + (a[..., 1] + b[..., 1])) + (a[..., 2] + b[..., 2])
        e = d / (np.float64(1.0e-4) + np.sqrt(np.float64(0.5) * s))
    e = np.where(ok, e, 0.0)
    pad = np.zeros((ty * th, tx * tw), np.float64)
    pad[:rows, :width] = e
    return pad.reshape(ty, th, tx, tw).max(axis=(1, 3))


def tile_view(a, t, grid):
    """the pixels of tile t of a [rows, width, ...] array"""
    tw, th, tx, _ = grid
    by, bx = divmod(int(t), tx)
    return a[by * th:(by + 1) * th, bx * tw:(bx + 1) * tw]


# ---------------------------------------------------------------------------------------------------- no GPU needed

def test_adaptive_calls_are_declared_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    for lib in (pkg.hip.LIB_PATH, pkg.hip.PROBE_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if l.split()}
        for n in NEW:
            assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} not declared in rt_abi.h"
            assert n in exported, f"{n} not exported by {os.path.basename(lib)}"


def test_adaptive_calls_refuse_null_arguments(pkg, abi):
    import ctypes as C
    L = pkg.hip.lib()
    out4 = (C.c_uint32 * 4)()
    assert L.rt_hip_tile_grid(None, None, out4) == abi.RT_ERR_INVALID
    assert L.rt_hip_accumulate_tiles(None, None, None, 1, 0, 8, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_tile_error(None, None, None, 1, None, 8, None, 4, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_resolve_tiles(None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_render_adaptive_to_host(None, 0.01, 16, None, None, None) == abi.RT_ERR_INVALID


def test_cli_adaptive_arguments(pkg, tmp_path):
    out = str(tmp_path / "o.png")
    cfg = "scenes/cfg1_test_800x600_spp16.json"
    for bad in (["--adaptive", "-1"], ["--adaptive", "x"], ["--adaptive", "nan"], ["--adaptive", "inf"], ["--adaptive"],
                ["--adaptive", "0.1", "--min-spp", "0"], ["--adaptive", "0.1", "--min-spp", "y"], ["--adaptive", "0.1", "--min-spp", "-3"],
                ["--min-spp", "8"], ["--adaptive", "0.1", "--passes", "2"], ["--passes", "2", "--adaptive", "0.1"],
                ["--adaptive", "0.1", "--frames", "3"], ["--frames", "3", "--adaptive", "0.1"], ["--adaptive", "0.1", "--orbit", "10"]):
        r = _cli([cfg, out, *bad])
        assert r.returncode == 0 and r.stdout.startswith("Usage: "), (bad, r.returncode, r.stdout, r.stderr)
    env = dict(os.environ, RT_GPUS="2")
    r = _cli([cfg, out, "--adaptive", "0.05"], env=env)
    assert r.returncode == 101 and len(r.stderr.strip().splitlines()) == 1 and "RT_GPUS" in r.stderr, (r.returncode, r.stderr)
    if not _has_gpu():   # without a GPU the run gets as far as the scene upload (before this feature: the usage line, exit 0)
        r = _cli([cfg, out, "--adaptive", "0.05", "--min-spp", "4"])
        assert r.returncode == 101 and not r.stdout.startswith("Usage"), (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _sync(torch):
    torch.cuda.current_stream().synchronize()


def _dev(torch, a):
    """numpy uint64 / uint32 / float64 array -> device tensor of the same bytes"""
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.float64): np.float64}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to("cuda:0")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _one_shot(torch, gs, spp, tiles=None, abi=None):
    rows = abi.tiles_local_rows(gs.height, tiles) if tiles is not None else gs.height
    gs.set_option("samples_per_pixel", spp)
    rgb = torch.zeros((rows, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((rows, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.render(rgb.data_ptr(), lin.data_ptr(), tiles, _stream(torch))
    gs.wait()
    return rgb.cpu().numpy(), lin.cpu().numpy()


def _accum_whole(torch, gs, rows, b, c, tiles=None):
    acc = torch.zeros((rows, gs.width, 3), dtype=torch.int64, device="cuda:0")
    gs.accumulate(acc.data_ptr(), b, c, tiles, _stream(torch))
    gs.wait()
    return _host(acc, np.uint64)


def _list_launch_matches(torch, pkg, abi, scene, opts=(), tiles=None, ranges=((0, 3), (3, 7)), what=""):
    gs = pkg.hip.HipScene(scene.ptr, 0)
    for k, v in opts:
        gs.set_option(k, v)
    rows = abi.tiles_local_rows(gs.height, tiles) if tiles is not None else gs.height
    grid = gs.tile_grid(tiles)
    tw, th, tx, ty = grid
    nt = tx * ty
    assert tx == -(-gs.width // tw) and ty == -(-rows // th), (grid, gs.width, rows)
    listed = np.arange(1, nt, 3, dtype=np.uint32)
    ids = np.concatenate([listed[::-1], np.array([nt, nt + 7, 0xFFFFFFFF], np.uint32)])[:nt]   # (out-of-range ids are skipped)
    listed = np.array([t for t in ids if t < nt], np.uint32)
    guard = np.full((rows, gs.width, 3), GUARD, np.uint64)
    for t in listed:
        tile_view(guard, t, grid)[...] = 0
    acc = _dev(torch, guard)
    d_list = _dev(torch, ids)
    for b, e in ranges:
        gs.accumulate_tiles(d_list.data_ptr(), len(ids), acc.data_ptr(), b, e - b, tiles, _stream(torch))
        gs.wait()
    got = _host(acc, np.uint64)
    whole = _accum_whole(torch, gs, rows, ranges[0][0], ranges[-1][1] - ranges[0][0], tiles)
    want = np.full_like(guard, GUARD)
    for t in listed:
        tile_view(want, t, grid)[...] = tile_view(whole, t, grid)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} words differ (grid {grid})"
    gs.close()


@pytest.mark.gpu
def test_list_launches_cover_and_lit(pkg, abi, torch_cuda, load_scene):
    _list_launch_matches(torch_cuda, pkg, abi, load_scene("cover", 120, 80, 8), what="cover 120x80")
    _list_launch_matches(torch_cuda, pkg, abi, load_scene("test", 80, 60, 8), what="lit 80x60")
    _list_launch_matches(torch_cuda, pkg, abi, load_scene("test", 80, 60, 8), opts=(("light_pool", 32), ("light_base_pool", 32)),
                         what="lit 80x60, pools of 32")


@pytest.mark.gpu
def test_list_launches_textured_brute_force_and_shards(pkg, abi, torch_cuda, load_scene):
    _list_launch_matches(torch_cuda, pkg, abi, load_scene("cover4k_tex", 64, 36, 6), what="textured 64x36")
    _list_launch_matches(torch_cuda, pkg, abi, load_scene("cover", 96, 64, 8), opts=(("variant", 1),), what="variant 1")
    for r in range(3):
        _list_launch_matches(torch_cuda, pkg, abi, load_scene("cover", 96, 64, 8), tiles=abi.RtRowTiles(2, r, 3), what=f"row tiles {{2, {r}, 3}}")
    for tl, shape in ((3, 0), (2, 1), (1, 2), (3, 3), (0, 0)):
        _list_launch_matches(torch_cuda, pkg, abi, load_scene("cover", 37, 23, 5), opts=(("tile_log2", tl), ("tile_shape", shape)),
                             ranges=((0, 5),), what=f"37x23 tile_log2 {tl} shape {shape}")


@pytest.mark.gpu
def test_list_launch_refusals(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    sc = load_scene("cover", 64, 48, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    tw, th, tx, ty = gs.tile_grid()
    acc = torch.zeros((48, 64, 3), dtype=torch.int64, device="cuda:0")
    d_list = _dev(torch, np.arange(tx * ty + 1, dtype=np.uint32))
    err = torch.zeros(tx * ty, dtype=torch.float64, device="cuda:0")
    for args in ((0, 1), (d_list.data_ptr(), 0), (d_list.data_ptr(), tx * ty + 1)):
        with pytest.raises(pkg.host.RtError) as e:
            gs.accumulate_tiles(*args, acc.data_ptr(), 0, 4, stream=_stream(torch))
        assert e.value.code == abi.RT_ERR_INVALID, args
        with pytest.raises(pkg.host.RtError) as e:
            gs.tile_error(*args, acc.data_ptr(), 8, acc.data_ptr(), 4, err.data_ptr(), stream=_stream(torch))
        assert e.value.code == abi.RT_ERR_INVALID, args
    for n_now, n_prev in ((4, 4), (4, 0), (3, 4)):
        with pytest.raises(pkg.host.RtError) as e:
            gs.tile_error(d_list.data_ptr(), 1, acc.data_ptr(), n_now, acc.data_ptr(), n_prev, err.data_ptr(), stream=_stream(torch))
        assert e.value.code == abi.RT_ERR_INVALID
    for thr, m, code in ((float("nan"), 16, abi.RT_ERR_INVALID), (-1e-9, 16, abi.RT_ERR_INVALID), (float("inf"), 16, abi.RT_ERR_INVALID),
                         (0.1, 0, abi.RT_ERR_INVALID)):
        with pytest.raises(pkg.host.RtError) as e:
            gs.render_adaptive(thr, m)
        assert e.value.code == code, (thr, m)
    gs.set_option("samples_per_pixel", 1 << 23)
    with pytest.raises(pkg.host.RtError) as e:
        gs.render_adaptive(0.1, 16)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
    _sync(torch)
    assert not acc.any().item()
    gs.close()


def _tile_error_dev(torch, gs, ids, now, n_now, prev, n_prev, nt, tiles=None):
    err = _dev(torch, np.full(nt, -7.0, np.float64))
    d_list = _dev(torch, np.asarray(ids, np.uint32))
    d_now, d_prev = _dev(torch, now), _dev(torch, prev)
    gs.tile_error(d_list.data_ptr(), len(ids), d_now.data_ptr(), n_now, d_prev.data_ptr(), n_prev, err.data_ptr(), tiles, _stream(torch))
    _sync(torch)
    return _host(err, np.float64)


def _check_errors(torch, gs, ids, now, n_now, prev, n_prev, rows, tiles=None, what=""):
    grid = gs.tile_grid(tiles)
    tw, th, tx, ty = grid
    nt = tx * ty
    got = _tile_error_dev(torch, gs, ids, now, n_now, prev, n_prev, nt, tiles)
    want = np_tile_error(now, prev, n_now, n_prev, grid, rows, gs.width).reshape(-1)
    listed = np.zeros(nt, bool)
    listed[[t for t in ids if t < nt]] = True
    assert np.all(got[~listed] == -7.0), f"{what}: unlisted entries written"
    assert np.array_equal(got[listed].view(np.uint64), want[listed].view(np.uint64)), \
        f"{what}: {int((got[listed] != want[listed]).sum())} tile errors differ (grid {grid}): {got[listed][:4]} vs {want[listed][:4]}"
    return want


@pytest.mark.gpu
def test_tile_error_rendered_accumulators(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    for name, w, h in (("cover", 120, 80), ("test", 80, 60), ("cover", 1, 40)):
        sc = load_scene(name, w, h, 16)
        gs = pkg.hip.HipScene(sc.ptr, 0)
        prev = _accum_whole(torch, gs, h, 0, 5)
        rest = _accum_whole(torch, gs, h, 5, 11)
        now = ((prev | rest) & F) | ((prev & ~F) + (rest & ~F))   # (the merge rule of include/rt_abi.h)
        tw, th, tx, ty = gs.tile_grid()
        e = _check_errors(torch, gs, list(range(tx * ty)), now, 16, prev, 5, h, what=f"{name} {w}x{h}")
        if w > 1:
            assert e.max() > 0
        else:
            assert (e == 0).all()   # (1 pixel wide: every sample NaN — nothing counts)
        gs.close()


@pytest.mark.gpu
def test_tile_error_crafted_words(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    for (w, h), tl, shape in (((37, 23), 0, 0), ((37, 23), 1, 0), ((37, 23), 1, 2), ((37, 23), 2, 1), ((37, 23), 3, 0), ((37, 23), 3, 3),
                              ((70, 9), 3, 2), ((5, 70), 2, 0), ((64, 64), 3, 0), ((129, 3), 3, 1)):
        sc = load_scene("cover", w, h, 4)
        gs = pkg.hip.HipScene(sc.ptr, 0)
        gs.set_option("tile_log2", tl)
        gs.set_option("tile_shape", shape)
        tw, th, tx, ty = gs.tile_grid()
        nt = tx * ty
        ids = list(range(nt - 1, -1, -2)) + [nt + 3]
        for n_prev, n_now in ((1, 2), (8, 16), (16, 29), ((1 << 22), (1 << 23) - 1)):
            top_p, top_b = n_prev << 40, (n_now - n_prev) << 40
            P = (rng.random((h, w, 3)) * top_p).astype(np.uint64)
            Q = P + (rng.random((h, w, 3)) * top_b).astype(np.uint64)
            P[rng.random((h, w, 3)) < 0.1] = 0
            Q[:2] = P[:2]                                          # equal halves
            Q[:, :1] = P[:, :1] * np.uint64(2) if n_now == 2 * n_prev else Q[:, :1]
            Q[rng.random((h, w, 3)) < 0.02] |= F                   # NaN flags in either buffer
            P[rng.random((h, w, 3)) < 0.02] |= F
            Q[-1] = 0; P[-1] = 0                                   # zeros
            _check_errors(torch, gs, ids, Q, n_now, P, n_prev, h, what=f"{w}x{h} tl {tl} shape {shape} n {n_prev}/{n_now}")
        gs.close()


def _resolve_tiles(torch, gs, acc, counts, tiles=None):
    rgb = torch.zeros(tuple(acc.shape), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros(tuple(acc.shape), dtype=torch.float32, device="cuda:0")
    d = _dev(torch, np.asarray(counts, np.uint32).reshape(-1))
    gs.resolve_tiles(acc.data_ptr(), d.data_ptr(), rgb.data_ptr(), lin.data_ptr(), tiles, _stream(torch))
    _sync(torch)
    return rgb.cpu().numpy(), lin.cpu().numpy()


def _resolve(torch, gs, acc, n, tiles=None):
    rgb = torch.zeros(tuple(acc.shape), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros(tuple(acc.shape), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), n, rgb.data_ptr(), lin.data_ptr(), tiles, _stream(torch))
    _sync(torch)
    return rgb.cpu().numpy(), lin.cpu().numpy()


@pytest.mark.gpu
def test_resolve_tiles(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    for name, w, h, opts, tiles in (("cover", 120, 80, (), None), ("cover", 1, 40, (), None), ("cover", 37, 23, (("tile_log2", 1),), None),
                                    ("cover", 37, 23, (("tile_log2", 2), ("tile_shape", 1)), None), ("cover", 96, 64, (), "shard")):
        sc = load_scene(name, w, h, 16)
        gs = pkg.hip.HipScene(sc.ptr, 0)
        for k, v in opts:
            gs.set_option(k, v)
        t = abi.RtRowTiles(2, 1, 3) if tiles else None
        rows = abi.tiles_local_rows(h, t) if t is not None else h
        grid = gs.tile_grid(t)
        tw, th, tx, ty = grid
        acc = _dev(torch, _accum_whole(torch, gs, rows, 0, 16, t))
        uni = _resolve_tiles(torch, gs, acc, np.full(tx * ty, 16), t)
        want = _resolve(torch, gs, acc, 16, t)
        assert np.array_equal(uni[0], want[0]) and np.array_equal(uni[1].view(np.uint32), want[1].view(np.uint32)), f"{name} {w}x{h}: uniform"
        counts = rng.choice([1, 3, 16, 77, (1 << 23) - 1], size=tx * ty)
        mixed = _resolve_tiles(torch, gs, acc, counts, t)
        for c in np.unique(counts):
            ref = _resolve(torch, gs, acc, int(c), t)
            for tid in np.nonzero(counts == c)[0]:
                for k in (0, 1):
                    g, r = tile_view(mixed[k], tid, grid), tile_view(ref[k], tid, grid)
                    assert np.array_equal(g.view(np.uint8 if k == 0 else np.uint32), r.view(np.uint8 if k == 0 else np.uint32)), (name, w, h, tid, c)
        gs.close()


def _pixels_per_tile(grid, rows, width):
    tw, th, tx, ty = grid
    cw = np.minimum(tw, width - np.arange(tx) * tw)
    ch = np.minimum(th, rows - np.arange(ty) * th)
    return np.outer(ch, cw)


def _tiles_match_one_shot(torch, abi, gs_ref, img, n_t, grid, lin=None, what=""):
    for c in np.unique(n_t):
        rgb_c, lin_c = _one_shot(torch, gs_ref, int(c), abi=abi)
        for tid in np.nonzero(n_t.reshape(-1) == c)[0]:
            assert np.array_equal(tile_view(img, tid, grid), tile_view(rgb_c, tid, grid)), f"{what}: tile {tid} at {c} samples (RGB8)"
            if lin is not None:
                assert np.array_equal(tile_view(lin, tid, grid).view(np.uint32), tile_view(lin_c, tid, grid).view(np.uint32)), \
                    f"{what}: tile {tid} at {c} samples (linear)"


@pytest.mark.gpu
def test_host_form_tiles_are_one_shot_frames(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    sc = load_scene("cover", 160, 96, 64)
    gs, ref = pkg.hip.HipScene(sc.ptr, 0), pkg.hip.HipScene(sc.ptr, 0)
    grid = gs.tile_grid()
    img, n_t, st = gs.render_adaptive(0.05, 8)
    assert n_t.shape == (grid[3], grid[2])
    assert set(np.unique(n_t)) <= {8, 16, 32, 64}, np.unique(n_t)
    _tiles_match_one_shot(torch, abi, ref, img, n_t, grid, what="cover 160x96 E 0.05")
    assert st["samples"] == int((_pixels_per_tile(grid, 96, 160) * n_t).sum())
    rounds = gs.adaptive_rounds()
    assert rounds[0][:2] == (n_t.size, 8) and all(r[2] > 0 for r in rounds), rounds
    img2, n_t2, _ = gs.render_adaptive(0.05, 8)   # deterministic
    assert np.array_equal(img, img2) and np.array_equal(n_t, n_t2)
    gs.close(); ref.close()


@pytest.mark.gpu
def test_host_form_limits(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    for n, m in ((13, 16), (37, 8), (1, 16), (16, 1)):   # E = 0: the one-shot frame (37 with M 8: 8 16 32 37; M < 2: one shot)
        sc = load_scene("cover", 72, 40, n)
        gs = pkg.hip.HipScene(sc.ptr, 0)
        img, n_t, st = gs.render_adaptive(0.0, m)
        want, _ = gs.render_to_host()
        assert np.array_equal(img, want) and (n_t == n).all(), (n, m)
        assert st["samples"] == 72 * 40 * n
        if n == 37:
            assert [r[1] for r in gs.adaptive_rounds()] == [8, 16, 32, 37]
        gs.close()
    sc = load_scene("cover", 72, 40, 64)     # a huge E: every tile stops at M
    gs = pkg.hip.HipScene(sc.ptr, 0)
    img, n_t, st = gs.render_adaptive(1e300, 8)
    gs.set_option("samples_per_pixel", 8)
    want, _ = gs.render_to_host()
    assert np.array_equal(img, want) and (n_t == 8).all() and st["samples"] == 72 * 40 * 8
    gs.close()
    sc = load_scene("cover", 40, 24, 32, depth=0)   # max_depth 0: black, every error 0
    gs = pkg.hip.HipScene(sc.ptr, 0)
    img, n_t, st = gs.render_adaptive(1e-12, 8)
    assert not img.any() and (n_t == 8).all() and st["segments"] == 0
    gs.close()
    sc = load_scene("cover", 1, 40, 32)      # 1 pixel wide: NaN samples count for nothing
    gs, ref = pkg.hip.HipScene(sc.ptr, 0), pkg.hip.HipScene(sc.ptr, 0)
    img, n_t, _ = gs.render_adaptive(1e-6, 4)
    assert (n_t == 4).all()
    _tiles_match_one_shot(torch, abi, ref, img, n_t, gs.tile_grid(), what="1 pixel wide")
    gs.close(); ref.close()


@pytest.mark.gpu
def test_schedule_replay_and_oracle_words(pkg, abi, oracle, torch_cuda, load_scene):
    """§3 replayed here with errors recomputed in numpy from accumulators rendered through accumulate_tiles; the words of each tile
    equal oracle.accumulate over [0, n_t), and the resolve of each tile is the one-shot frame at n_t (RGB8 and linear)"""
    torch = torch_cuda
    N, M, E = 40, 8, 0.08
    sc = load_scene("cover", 48, 32, N)
    gs, ref = pkg.hip.HipScene(sc.ptr, 0), pkg.hip.HipScene(sc.ptr, 0)
    for k, v in (("tile_log2", 1),):   # (2x2 -> 4x1 strips: many tiles on a small window)
        gs.set_option(k, v); ref.set_option(k, v)
    img, n_host, _ = gs.render_adaptive(E, M)
    grid = gs.tile_grid()
    tw, th, tx, ty = grid
    nt = tx * ty
    rows, w = 32, 48
    now = torch.zeros((rows, w, 3), dtype=torch.int64, device="cuda:0")
    everything = list(range(nt))
    d_all = _dev(torch, np.array(everything, np.uint32))
    h = M // 2
    gs.accumulate_tiles(d_all.data_ptr(), nt, now.data_ptr(), 0, h, None, _stream(torch)); gs.wait()
    prev = now.clone()
    gs.accumulate_tiles(d_all.data_ptr(), nt, now.data_ptr(), h, M - h, None, _stream(torch)); gs.wait()
    n_t = np.full(nt, M, np.uint32)
    active, n, n_prev = everything, M, h
    while n < N:
        hn, hp = _host(now, np.uint64), _host(prev, np.uint64)
        e = _check_errors(torch, gs, active, hn, n, hp, n_prev, rows, what=f"round at {n}")
        active = [t for t in active if e[t] >= E]
        if not active:
            break
        add = min(n, N - n)
        prev = now.clone()
        d = _dev(torch, np.array(active, np.uint32))
        gs.accumulate_tiles(d.data_ptr(), len(active), now.data_ptr(), n, add, None, _stream(torch)); gs.wait()
        n_prev, n = n, n + add
        n_t[active] = n
    assert np.array_equal(n_t.reshape(ty, tx), n_host), (n_t.reshape(ty, tx), n_host)
    words = _host(now, np.uint64)
    for c in np.unique(n_t):
        o, _ = oracle.accumulate(abi, sc.ptr, 0, int(c))
        for tid in np.nonzero(n_t == c)[0]:   # (the GPU's sums against the CPU's: flags identical, sums within the parity bar on the mean)
            g, r = tile_view(words, tid, grid), tile_view(o, tid, grid)
            assert np.array_equal(g & F, r & F), f"tile {tid}: NaN flags at {c} samples differ from the oracle"
            d = np.abs((g & ~F).astype(np.int64) - (r & ~F).astype(np.int64)).max()
            assert d <= int(c) * (1 << 40) * LINEAR_ATOL, f"tile {tid}: sums at {c} samples differ from the oracle by {d}"
    rgb, lin = _resolve_tiles(torch, gs, now, n_t)
    assert np.array_equal(rgb, img)
    _tiles_match_one_shot(torch, abi, ref, rgb, n_t, grid, lin=lin, what="replay 48x32")
    gs.close(); ref.close()


@pytest.mark.gpu
def test_cli_adaptive(pkg, host, abi, torch_cuda, load_scene, tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")))
    cfg.update(width=120, height=80, samples_per_pixel=32)
    path = tmp_path / "small.json"
    path.write_text(json.dumps(cfg))
    one, ad0, ad = str(tmp_path / "one.png"), str(tmp_path / "ad0.png"), str(tmp_path / "ad.png")
    r1 = _cli([str(path), one])
    r0 = _cli([str(path), ad0, "--adaptive", "0"])
    assert r1.returncode == 0 and r0.returncode == 0, (r1.stderr, r0.stderr)
    assert open(one, "rb").read() == open(ad0, "rb").read(), "--adaptive 0 is not the one-shot PNG"
    assert re.fullmatch(r"\nRendering " + re.escape(ad0) + r"\nFrame time: \d+ms\n", r0.stdout), r0.stdout
    rounds = [l for l in r0.stderr.splitlines() if l.startswith("round ")]
    assert [re.match(r"round (\d+): \d+ tiles at (\d+) samples, kernel [\d.]+ ms$", l).groups() for l in rounds] == \
        [("0", "16"), ("1", "32")], r0.stderr
    assert re.search(r"samples traced, 1\.0000 of 120x80x32", r0.stderr), r0.stderr
    r = _cli([str(path), ad, "--adaptive", "0.05", "--min-spp", "8"])
    assert r.returncode == 0, r.stderr
    sc = load_scene(str(path))
    gs = pkg.hip.HipScene(sc.ptr, 0)
    img, n_t, _ = gs.render_adaptive(0.05, 8)
    host.png_write(str(tmp_path / "want.png"), img)
    assert open(ad, "rb").read() == open(str(tmp_path / "want.png"), "rb").read()
    _tiles_match_one_shot(torch_cuda, abi, gs, img, n_t, gs.tile_grid(), what="CLI 120x80")
    gs.close()
