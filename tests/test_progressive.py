"""Progressive rendering (include/rt_abi.h rt_hip_accumulate / rt_hip_resolve / rt_hip_refine_to_host, the CLI's --passes):
a frame's samples rendered in passes, added up exactly in a u64 accumulator and resolved at any point.

Sample s of pixel p traces the same path whatever the frame's sample count, and pixel sums are exact fixed point, so every
split of [0, N) — any sizes, any order, any row tiles, any number of scenes — resolved over N is the one-shot frame at N
samples BIT FOR BIT: RGB8, linear radiance (NaN pixels included) and the path counters summed over the passes."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from parity import assert_parity, pooled_atol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_hip_accumulate", "rt_hip_resolve", "rt_hip_refine_to_host")
F = np.uint64(1 << 63)   # sticky NaN flag of an accumulator word
MAX_SAMPLES = (1 << 23) - 1


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---------------------------------------------------------------------------------------------------- no GPU needed

def test_progressive_calls_are_declared_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    for lib in (pkg.hip.LIB_PATH, pkg.hip.PROBE_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if l.split()}
        for n in NEW:
            assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} not declared in rt_abi.h"
            assert n in exported, f"{n} not exported by {os.path.basename(lib)}"


def test_progressive_calls_refuse_null_arguments(pkg, abi, load_scene):
    L = pkg.hip.lib()
    assert L.rt_hip_accumulate(None, None, 0, 8, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_resolve(None, None, None, 8, None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_refine_to_host(None, 8, None, None) == abi.RT_ERR_INVALID
    if _has_gpu():
        return
    sc = load_scene("cover", 16, 16, 4)
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0)
    assert e.value.code == abi.RT_ERR_NO_DEVICE


def _cli(args, env=None):
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    return subprocess.run([exe, *args], capture_output=True, text=True, cwd=ROOT, timeout=120, env=env)


def test_cli_passes_arguments(pkg, tmp_path):
    out = str(tmp_path / "o.png")
    cfg = "scenes/cfg1_test_800x600_spp16.json"
    for bad in (["--passes", "0"], ["--passes", "x"], ["--passes", "-2"], ["--passes", "2", "--frames", "3"], ["--frames", "3", "--passes", "2"],
                ["--passes", "17"], ["--passes"]):
        r = _cli([cfg, out, *bad])
        assert r.returncode == 0 and r.stdout.startswith("Usage: "), (bad, r.returncode, r.stdout, r.stderr)
    env = dict(os.environ, RT_GPUS="2")
    r = _cli([cfg, out, "--passes", "4"], env=env)
    assert r.returncode == 101 and len(r.stderr.strip().splitlines()) == 1 and "RT_GPUS" in r.stderr, (r.returncode, r.stderr)
    if not _has_gpu():   # without a GPU the run gets as far as the scene upload (before this feature: the usage line, exit 0)
        r = _cli([cfg, out, "--passes", "4"])
        assert r.returncode == 101 and not r.stdout.startswith("Usage"), (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _one_shot(torch, gs, spp, tiles=None, abi=None):
    rows = abi.tiles_local_rows(gs.height, tiles) if tiles is not None else gs.height
    gs.set_option("samples_per_pixel", spp)
    rgb = torch.zeros((rows, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((rows, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.render(rgb.data_ptr(), lin.data_ptr(), tiles, _stream(torch))
    st = gs.wait()
    return rgb.cpu().numpy(), lin.cpu().numpy(), st


def _new_accum(torch, gs, rows=None):
    return torch.zeros((gs.height if rows is None else rows, gs.width, 3), dtype=torch.int64, device="cuda:0")


def _accumulate(torch, gs, acc, ranges, tiles=None):
    """add the sample ranges [b, e) to acc, one pass each; returns the counters summed over the passes"""
    total = {}
    for b, e in ranges:
        gs.accumulate(acc.data_ptr(), b, e - b, tiles, _stream(torch))
        st = gs.wait()
        for k in ("segments", "exact_tests", "grid_steps", "tex_oob", "segments_repeated"):
            total[k] = total.get(k, 0) + st[k]
    return total


def _resolve(torch, gs, acc, n, tiles=None):
    rgb = torch.zeros(tuple(acc.shape), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros(tuple(acc.shape), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), n, rgb.data_ptr(), lin.data_ptr(), tiles, _stream(torch))
    torch.cuda.current_stream().synchronize()
    return rgb.cpu().numpy(), lin.cpu().numpy()


def _assert_identical(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: RGB8 differs at {int((got[0] != want[0]).sum())} values"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), f"{what}: linear radiance differs bitwise"


def _assert_counts(passes, one, what=""):
    assert passes["segments"] == one["segments"] and passes["tex_oob"] == one["tex_oob"], (what, passes, one)
    # a lit segment repeated for want of a free pool record counts its exact tests and grid steps twice; where the split moved
    # the repeats (the pool placement hashes the sample index) only the segments are comparable
    if passes["segments_repeated"] == 0 and one["segments_repeated"] == 0:
        assert passes["exact_tests"] == one["exact_tests"] and passes["grid_steps"] == one["grid_steps"], (what, passes, one)


def _split_equals_one_shot(torch, pkg, scene, ranges, opts=(), what=""):
    gs = pkg.hip.HipScene(scene.ptr, 0)
    for k, v in opts:
        gs.set_option(k, v)
    n = max(e for _, e in ranges)
    one = _one_shot(torch, gs, n, abi=pkg.abi)
    acc = _new_accum(torch, gs)
    counts = _accumulate(torch, gs, acc, ranges)
    got = _resolve(torch, gs, acc, n)
    _assert_identical(got, one, what)
    _assert_counts(counts, one[2], what)
    gs.close()
    return got, one, counts


@pytest.mark.gpu
def test_cover_passes_equal_one_shot_frames(pkg, abi, oracle, torch_cuda, load_scene):
    torch = torch_cuda
    sc = load_scene("cover", 240, 160, 32)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    one8 = _one_shot(torch, gs, 8, abi=abi)
    one32 = _one_shot(torch, gs, 32, abi=abi)
    acc = _new_accum(torch, gs)
    c8 = _accumulate(torch, gs, acc, [(0, 8)])
    _assert_identical(_resolve(torch, gs, acc, 8), one8, "after [0, 8)")
    _assert_counts(c8, one8[2], "after [0, 8)")
    c = _accumulate(torch, gs, acc, [(8, 16), (16, 32)])
    got = _resolve(torch, gs, acc, 32)
    _assert_identical(got, one32, "[0, 8) [8, 16) [16, 32)")
    _assert_counts({k: c8[k] + c[k] for k in c}, one32[2], "[0, 8) [8, 16) [16, 32)")
    o_rgb, o_lin, _ = oracle.render(abi, sc.ptr)
    assert_parity(got[0], got[1], o_rgb, o_lin, "progressive cover 240x160 spp 32", atol=pooled_atol(32))
    gs.close()


@pytest.mark.gpu
def test_out_of_order_uneven_passes(pkg, torch_cuda, load_scene):
    _split_equals_one_shot(torch_cuda, pkg, load_scene("cover", 120, 80, 32), [(20, 32), (0, 1), (1, 20)], what="[20,32) [0,1) [1,20)")


@pytest.mark.gpu
def test_lit_scene_passes(pkg, torch_cuda, load_scene):
    """lights, nested light rays, hollow glass; then pools so small that segments repeat"""
    sc = load_scene("test", 80, 60, 16)
    _split_equals_one_shot(torch_cuda, pkg, sc, [(0, 5), (5, 6), (6, 16)], what="lit 80x60")
    _, one, counts = _split_equals_one_shot(torch_cuda, pkg, sc, [(0, 5), (5, 6), (6, 16)], opts=(("light_pool", 32), ("light_base_pool", 32)),
                                            what="lit 80x60, pools of 32")
    assert one[2]["segments_repeated"] + counts["segments_repeated"] > 0, "the shrunk pools were never exhausted"


@pytest.mark.gpu
def test_textured_window_passes(pkg, torch_cuda, load_scene):
    _split_equals_one_shot(torch_cuda, pkg, load_scene("cover4k_tex", 64, 36, 6), [(0, 2), (2, 6)], what="textured 64x36")


@pytest.mark.gpu
def test_brute_force_variant_passes(pkg, torch_cuda, load_scene):
    _split_equals_one_shot(torch_cuda, pkg, load_scene("cover", 96, 64, 8), [(0, 3), (3, 8)], opts=(("variant", 1),), what="variant 1")


@pytest.mark.gpu
def test_edge_cases(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    # a frame one pixel wide: the camera's u = i / (width - 1) is NaN, so are the samples; the NaN pixels match
    got, _, _ = _split_equals_one_shot(torch, pkg, load_scene("cover", 1, 40, 8), [(0, 3), (3, 8)], what="1 pixel wide")
    assert np.isnan(got[1]).any()
    # max_depth 0: black, nothing traced
    got, _, counts = _split_equals_one_shot(torch, pkg, load_scene("cover", 32, 24, 8, depth=0), [(0, 5), (5, 8)], what="max_depth 0")
    assert not got[0].any() and counts["segments"] == 0
    # refused calls enqueue nothing: a normal frame after them is the frame
    sc = load_scene("cover", 64, 48, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    ref = _one_shot(torch, gs, 4, abi=abi)
    acc = _new_accum(torch, gs)
    for args, code in (((acc.data_ptr(), 0, 0), abi.RT_ERR_INVALID), ((acc.data_ptr(), MAX_SAMPLES - 1, 2), abi.RT_ERR_UNSUPPORTED),
                       ((acc.data_ptr() + 4, 0, 4), abi.RT_ERR_INVALID), ((0, 0, 4), abi.RT_ERR_INVALID)):
        with pytest.raises(pkg.host.RtError) as e:
            gs.accumulate(*args, stream=_stream(torch))
        assert e.value.code == code, args
    for n, code in ((0, abi.RT_ERR_INVALID), (MAX_SAMPLES + 1, abi.RT_ERR_UNSUPPORTED)):
        with pytest.raises(pkg.host.RtError) as e:
            gs.resolve(acc.data_ptr(), n, 0, stream=_stream(torch))
        assert e.value.code == code, n
    with pytest.raises(pkg.host.RtError) as e:
        gs.refine_to_host(0)
    assert e.value.code == abi.RT_ERR_INVALID
    assert not acc.any().item()
    _assert_identical(_one_shot(torch, gs, 4, abi=abi), ref, "frame after refused calls")
    gs.close()


@pytest.mark.gpu
def test_row_tiles_accumulate_and_assemble(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    sc = load_scene("cover", 96, 64, 8)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    one = _one_shot(torch, gs, 8, abi=abi)
    rgb = np.zeros_like(one[0])
    lin = np.full_like(one[1], -1.0)
    counts = {}
    for r in range(3):
        t = abi.RtRowTiles(2, r, 3)
        acc = _new_accum(torch, gs, abi.tiles_local_rows(gs.height, t))
        c = _accumulate(torch, gs, acc, [(0, 3), (3, 8)], tiles=t)
        counts = {k: counts.get(k, 0) + c[k] for k in c}
        g_rgb, g_lin = _resolve(torch, gs, acc, 8, tiles=t)
        rows = abi.tiles_global_rows(gs.height, t)
        rgb[rows], lin[rows] = g_rgb, g_lin
    _assert_identical((rgb, lin), one, "row tiles {2, r, 3}")
    _assert_counts(counts, one[2], "row tiles {2, r, 3}")
    gs.close()


@pytest.mark.gpu
def test_accumulators_of_two_scenes_merge(pkg, abi, torch_cuda, load_scene):
    """the accumulator layout is a contract: sums of disjoint ranges merge on the host with one formula"""
    torch = torch_cuda
    sc = load_scene("cover", 1, 24, 32)   # (NaN pixels: the flag survives the merge)
    sc2 = load_scene("cover", 96, 64, 32)
    for scene in (sc, sc2):
        a_gs, b_gs = pkg.hip.HipScene(scene.ptr, 0), pkg.hip.HipScene(scene.ptr, 0)
        one = _one_shot(torch, a_gs, 32, abi=abi)
        a, b = _new_accum(torch, a_gs), _new_accum(torch, b_gs)
        _accumulate(torch, a_gs, a, [(0, 16)])
        _accumulate(torch, b_gs, b, [(16, 32)])
        ha, hb = a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)
        merged = ((ha | hb) & F) | ((ha & ~F) + (hb & ~F))
        m = torch.from_numpy(merged.view(np.int64)).to("cuda:0")
        _assert_identical(_resolve(torch, a_gs, m, 32), one, f"merged {scene.c.width}x{scene.c.height}")
        a_gs.close(); b_gs.close()


@pytest.mark.gpu
def test_refine_to_host(pkg, abi, torch_cuda, load_scene):
    sc = load_scene("cover", 120, 80, 32)
    gs = pkg.hip.HipScene(sc.ptr, 0)    # the one-shot frames
    ps = pkg.hip.HipScene(sc.ptr, 0)    # the progressive one
    assert ps.query("accum_samples") == 0
    n = 0
    for k in (8, 8, 16):
        img, st = ps.refine_to_host(k)
        n += k
        assert ps.query("accum_samples") == n
        gs.set_option("samples_per_pixel", n)
        want, _ = gs.render_to_host()
        assert np.array_equal(img, want), n
    c = sc.c
    moved = [[c.cam_origin[i] + (0.3 if i == 0 else 0.0) for i in range(3)], [c.cam_lower_left[i] + (0.3 if i == 0 else 0.0) for i in range(3)],
             list(c.cam_horizontal), list(c.cam_vertical)]
    ps.set_camera(*moved)
    assert ps.query("accum_samples") == 0
    img, _ = ps.refine_to_host(32)
    gs.set_camera(*moved)
    gs.set_option("samples_per_pixel", 32)
    want, _ = gs.render_to_host()
    assert np.array_equal(img, want)
    ps.set_option("accum_reset", 1)
    assert ps.query("accum_samples") == 0
    with pytest.raises(pkg.host.RtError):
        ps.set_option("accum_reset", 0)
    gs.close(); ps.close()


@pytest.mark.gpu
def test_cli_passes(pkg, torch_cuda, tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")))
    cfg.update(width=120, height=80, samples_per_pixel=10)
    path = tmp_path / "small.json"
    path.write_text(json.dumps(cfg))
    one, prog = str(tmp_path / "one.png"), str(tmp_path / "prog.png")
    r1 = _cli([str(path), one])
    r3 = _cli([str(path), prog, "--passes", "3"])
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr, r3.stderr)
    assert open(one, "rb").read() == open(prog, "rb").read(), "the last pass's PNG is not the one-shot PNG"
    assert re.fullmatch(r"\nRendering " + re.escape(prog) + r"\nFrame time: \d+ms\n", r3.stdout), r3.stdout
    lines = [l for l in r3.stderr.splitlines() if l.startswith("pass ")]
    assert [l.split(":")[0] for l in lines] == ["pass 1/3", "pass 2/3", "pass 3/3"], r3.stderr
    assert [int(l.split(": ")[1].split()[0]) for l in lines] == [4, 3, 3]
    assert not os.path.exists(prog + ".part")
