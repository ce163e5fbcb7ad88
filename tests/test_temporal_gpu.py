"""Temporal denoising on the GPU (include/rt_abi.h rt_hip_reproject / rt_hip_render_frame_temporal_to_host / rt_hip_temporal_*, the
CLI's --frames N --orbit DEG --denoise).  rt_hip_reproject against tests/temporal_ref.py (numpy, written from the
header's text) bit for bit; the host form against the calls it is made of."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import temporal_cases as TC
import temporal_ref

try:   # (before librt_hip.so is loaded, as collecting the whole suite does: the process then holds ONE HIP runtime, torch's)
    import torch  # noqa: F401
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_FILES = {"cover": "scenes/cfg2_cover_1200x800_spp128.json", "test": "scenes/cfg1_test_800x600_spp16.json"}
F = np.float32
pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _orbit_camera(host, name, deg):
    """the scene file's camera turned by deg about the y axis around look_at (both scenes' vup), as 12 doubles"""
    cam = json.load(open(os.path.join(ROOT, SCENE_FILES[name])))["camera"]
    v = lambda k: np.array([cam[k]["x"], cam[k]["y"], cam[k]["z"]])
    d = host.camera_derive(list(TC.orbit(v("look_from"), v("look_at"), deg)), list(v("look_at")), list(v("vup")), cam["vfov"], cam["aspect"])
    return np.array(d["origin"] + d["lower_left_corner"] + d["horizontal"] + d["vertical"])


def _set_camera(gs, cam):
    gs.set_camera(list(cam[0:3]), list(cam[3:6]), list(cam[6:9]), list(cam[9:12]))


def _aovs(torch, gs, n):
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(n, aov.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    return aov


def _linear(torch, gs, begin, count):
    """samples [begin, begin + count) of every pixel resolved to linear f32, through rt_hip_accumulate and rt_hip_resolve"""
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    gs.accumulate(acc.data_ptr(), begin, count, stream=_stream(torch))
    gs.wait()
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), count, 0, lin.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    return lin


def _gpu_reproject(torch, gs, lin, aov, prev_hist, prev_aov, prev_cam, params):
    """rt_hip_reproject into a buffer with guard words on both sides"""
    h, w = gs.height, gs.width
    guard = torch.full((h * w * 4 + 8,), -7.0, dtype=torch.float32, device="cuda:0")
    gs.reproject(lin.data_ptr(), aov.data_ptr(), prev_hist.data_ptr(), prev_aov.data_ptr(), prev_cam, guard.data_ptr() + 16, params, stream=_stream(torch))
    torch.cuda.synchronize()
    g = guard.cpu().numpy()
    assert (g[:4] == -7.0).all() and (g[-4:] == -7.0).all(), "words outside d_out_history were written"
    return g[4:-4].reshape(h, w, 4)


def _same(got, want, what):
    bad = np.argwhere((_bits(got) != _bits(want)).any(-1))
    assert bad.size == 0, (what, len(bad), [(tuple(p), got[tuple(p)], want[tuple(p)]) for p in bad[:3]])


@pytest.mark.parametrize("name", ["cover", "test"])
def test_reproject_matches_numpy_on_real_frames(pkg, host, torch_cuda, load_scene, name):
    """8-spp colours and real guides at 96 x 64: the first frame against an empty history, the frame after a 3 degree orbit against
    it, and a second frame of that view against that"""
    torch = torch_cuda
    sc = load_scene(name, 96, 64, 8)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    cams = [_orbit_camera(host, name, 0.0), _orbit_camera(host, name, 3.0), _orbit_camera(host, name, 3.0)]
    for params in ((0.0, 1e30, 0.1, 0.05, 0.1), (0.2, 4.0, 1e30, 1e30, 1e30), (0.1, 32.0, 0.0, 0.0, 0.0)):
        prev_hist = torch.zeros((64, 96, 4), dtype=torch.float32, device="cuda:0")
        prev_aov = torch.zeros((64, 96, 8), dtype=torch.float32, device="cuda:0")
        prev_cam = cams[0]
        reused = []
        for f, cam in enumerate(cams):
            _set_camera(gs, cam)
            lin, aov = _linear(torch, gs, 8 * f, 8), _aovs(torch, gs, 8)
            got = _gpu_reproject(torch, gs, lin, aov, prev_hist, prev_aov, prev_cam, params)
            want = temporal_ref.reproject(lin.cpu().numpy(), aov.cpu().numpy(), prev_hist.cpu().numpy(), prev_aov.cpu().numpy(), cam, prev_cam, *params)
            _same(got, want, (name, params, f))
            reused.append(float((got[..., 3] > 1).mean()))
            prev_hist, prev_aov, prev_cam = _dev(torch, got), aov, cam
        assert reused[0] == 0.0, reused
        print(name, params, "pixels with history per frame:", reused)
        if params[2] > 0:    # (thresholds 0 ask for bit-equal guides and depths: an accident, even in a static view)
            assert reused[1] > 0.25 and reused[2] > 0.8, (name, params, reused)
    gs.close()


@pytest.mark.parametrize("h,w", TC.SIZES)
def test_reproject_matches_numpy_on_crafted_frames(pkg, torch_cuda, load_scene, h, w):
    torch = torch_cuda
    rng = np.random.default_rng(1000 * h + w)
    bufs = TC.crafted(rng, h, w)
    sc = load_scene("cover", w, h, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    d = [_dev(torch, b) for b in bufs]
    for name, (cam, prev_cam) in TC.camera_pairs().items():
        _set_camera(gs, cam)
        for params in TC.PARAMS:
            got = _gpu_reproject(torch, gs, *d, prev_cam, params)
            want = temporal_ref.reproject(*bufs, cam, prev_cam, *params)
            _same(got, want, (h, w, name, params))
    gs.close()


def test_static_camera_accumulates_the_running_mean(pkg, torch_cuda, load_scene):
    """eight frames of 4 spp, alpha_min = 0, no cap on n, no spatial filter: the history is the mean of samples [0, 32).  Per channel
    8 * 4 * 2^-24 * max(1, value): four f32 roundings per frame of the running mean (hist = s / sw, c - hist, alpha *, hist +); the
    bilinear weight that leaks to a neighbour is below 1e-12.  Fails if two frames trace the same sample range."""
    torch = torch_cuda
    sc = load_scene("cover", 96, 64, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.temporal_configure(0.0, 1e30, 0.1, 0.1, 0.1)
    for f in range(8):
        gs.render_frame_temporal_to_host(f, 0)
    hist = gs.temporal_history()
    want = _linear(torch, gs, 0, 32).cpu().numpy()
    gs.close()
    assert not np.isnan(want).any()
    err = np.abs(hist[..., 0:3].astype(np.float64) - want)
    bound = 8 * 4 * 2.0 ** -24 * np.maximum(1.0, want.astype(np.float64))
    print(f"running mean: max |history - mean of 32 samples| {err.max():.3e}, max of err / bound {float((err / bound).max()):.3f}")
    assert (hist[..., 3] == 8.0).all(), np.unique(hist[..., 3], return_counts=True)
    assert (err <= bound).all(), (float(err.max()), int((err > bound).sum()))


def test_camera_jump_drops_the_history(pkg, host, torch_cuda, load_scene):
    """a 90 degree jump with thresholds 0: the new frame alone, bit for bit, n = 1 at every pixel"""
    torch = torch_cuda
    sc = load_scene("cover", 96, 64, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.temporal_configure(0.1, 32.0, 0.0, 0.0, 0.0)
    gs.render_frame_temporal_to_host(0, 0)
    _set_camera(gs, _orbit_camera(host, "cover", 90.0))
    gs.render_frame_temporal_to_host(1, 0)
    hist = gs.temporal_history()
    want = _linear(torch, gs, 4, 4).cpu().numpy()      # frame 1 of 4 spp traces samples [4, 8)
    gs.close()
    assert not np.isnan(want).any()
    assert np.array_equal(_bits(hist[..., 0:3]), _bits(want)) and (hist[..., 3] == 1.0).all()


def test_moved_sphere_drops_the_history_it_covers(pkg, abi, torch_cuda, load_scene):
    """the large metal sphere moved onto pixels that showed the ground: there the albedo of the guides changed by more than tau_a, so
    those pixels start over (n = 1) while the ground around keeps its history (n = 2); no motion vectors are involved"""
    torch = torch_cuda
    sc = load_scene("cover", 96, 64, 4)
    n = sc.c.n_spheres
    centres = np.array([[sc.c.spheres[i].center[k] for k in range(3)] for i in range(n)])
    assert np.allclose(centres[n - 1], (4.0, 1.0, 0.0)) and sc.c.spheres[n - 1].kind == abi.RT_MAT_METAL
    metal = np.array([sc.c.spheres[n - 1].albedo[k] for k in range(3)], F)
    ground = np.array([sc.c.spheres[0].albedo[k] for k in range(3)], F)
    tau_a = 0.01
    assert float(((metal - ground) ** 2).sum()) > 2 * tau_a
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.temporal_configure(0.0, 1e30, 1e30, tau_a, 1e30)      # (the albedo test alone decides)
    before = _aovs(torch, gs, 4).cpu().numpy()
    gs.render_frame_temporal_to_host(0, 0)
    moved = centres.copy()
    moved[n - 1] = (4.0, 1.0, 2.5)
    gs.update_spheres(moved)
    after = _aovs(torch, gs, 4).cpu().numpy()
    gs.render_frame_temporal_to_host(1, 0)
    hist = gs.temporal_history()
    gs.close()
    was_ground = (before[..., 7] == 1.0) & (before[..., 0:3] == ground).all(-1)
    is_metal = (after[..., 7] == 1.0) & (after[..., 0:3] == metal).all(-1)
    covered = was_ground & is_metal
    assert covered.sum() >= 20, int(covered.sum())
    assert (hist[covered][:, 3] == 1.0).all(), np.unique(hist[covered][:, 3], return_counts=True)
    still_ground = was_ground & (after[..., 7] == 1.0) & (after[..., 0:3] == ground).all(-1)
    assert still_ground.sum() > 500 and (hist[still_ground][:, 3] == 2.0).mean() > 0.95


def test_frame_zero_is_the_denoised_one_shot_frame(pkg, torch_cuda, load_scene):
    sc = load_scene("cover", 96, 64, 8)
    ref = pkg.hip.HipScene(sc.ptr, 0)
    want, _ = ref.refine_to_host_denoised(8, 2)
    ref.close()
    gs = pkg.hip.HipScene(sc.ptr, 0)
    got, st = gs.render_frame_temporal_to_host(0, 2)
    assert np.array_equal(got, want)
    assert st["samples"] == 96 * 64 * 8 and st["kernel_ms"] > 0
    # ... and the history starts over after a reset, and in a new scene
    later = [gs.render_frame_temporal_to_host(f, 2)[0] for f in (1, 2)]
    assert not np.array_equal(later[1], want)
    assert (gs.temporal_history()[..., 3] == 3.0).mean() > 0.9
    gs.temporal_reset()
    with pytest.raises(pkg.host.RtError):
        gs.temporal_history()
    assert np.array_equal(gs.render_frame_temporal_to_host(0, 2)[0], want)
    assert (gs.temporal_history()[..., 3] == 1.0).all()
    gs.close()
    gs = pkg.hip.HipScene(sc.ptr, 0)
    assert np.array_equal(gs.render_frame_temporal_to_host(0, 2)[0], want)
    gs.close()


def test_temporal_frames_leave_nothing_behind(pkg, torch_cuda, load_scene):
    """a plain frame and a progressive pass rendered after temporal frames are the ones rendered before them: queue order, counters
    and the progressive accumulator are untouched"""
    sc = load_scene("cover", 96, 64, 6)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    plain, _ = gs.render_to_host()
    first, _ = gs.refine_to_host(3)
    for f in range(3):
        gs.render_frame_temporal_to_host(f, 2)
    assert np.array_equal(gs.render_to_host()[0], plain)
    assert gs.query("accum_samples") == 3
    second, _ = gs.refine_to_host(3)
    gs.close()
    fresh = pkg.hip.HipScene(sc.ptr, 0)
    assert np.array_equal(fresh.refine_to_host(6)[0], second) and not np.array_equal(first, second)
    fresh.close()


def test_temporal_calls_refuse_bad_arguments_on_a_scene(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    h, w = 24, 32
    sc = load_scene("cover", w, h, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    aov, paov = (torch.zeros((h, w, 8), dtype=torch.float32, device="cuda:0") for _ in range(2))
    hist = torch.zeros((h * w * 4 + 8,), dtype=torch.float32, device="cuda:0")
    out = torch.full((h * w * 4 + 8,), 7.0, dtype=torch.float32, device="cuda:0")
    L, s = pkg.hip.lib(), gs._h
    cam = (C.c_double * 12)(*TC.camera_pairs()["identical"][0])
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    good = (0.1, 32.0, 0.1, 0.1, 0.1)

    def call(lin_=p(lin), aov_=p(aov), hist_=p(hist), paov_=p(paov), cam_=cam, k=good, out_=p(out)):
        return L.rt_hip_reproject(s, lin_, aov_, hist_, paov_, cam_, *k, out_, None)
    cases = [call(lin_=None), call(aov_=None), call(hist_=None), call(paov_=None), call(cam_=None), call(out_=None),
             call(lin_=p(lin, 2)), call(aov_=p(aov, 4)), call(hist_=p(hist, 8)), call(paov_=p(paov, 4)), call(out_=p(out, 8)),
             call(out_=p(hist)), call(out_=p(hist, 16)), call(out_=p(lin)), call(out_=p(aov)), call(out_=p(paov))]      # overlaps
    for i in range(2, 5):
        for bad in (-1.0, float("nan"), float("inf")):
            cases.append(call(k=good[:i] + (bad,) + good[i + 1:]))
    for bad in (-0.01, 1.01, float("nan")):
        cases.append(call(k=(bad,) + good[1:]))
    for bad in (0.5, 0.0, -1.0, float("nan")):
        cases.append(call(k=good[:1] + (bad,) + good[2:]))
        cases.append(L.rt_hip_temporal_configure(s, good[0], bad, *good[2:]))
    cases.append(L.rt_hip_temporal_configure(s, 2.0, *good[1:]))
    cases.append(L.rt_hip_temporal_configure(s, *good[:4], float("inf")))
    for i, rc in enumerate(cases):
        assert rc == abi.RT_ERR_INVALID, (i, rc)
    host_out = np.zeros((h, w, 3), np.uint8)
    assert L.rt_hip_render_frame_temporal_to_host(s, 0, 9, host_out.ctypes.data_as(C.c_void_p), None) == abi.RT_ERR_UNSUPPORTED
    assert L.rt_hip_render_frame_temporal_to_host(s, 0, 2, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_temporal_history(s, host_out.ctypes.data_as(C.c_void_p)) == abi.RT_ERR_INVALID      # no history yet
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all(), "a refused call wrote its output"
    assert call() == abi.RT_OK and call(k=(0.0, float("inf"), 0.0, 0.0, 0.0)) == abi.RT_OK      # (and the good call is good)
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[: h * w * 4] != 7.0).all()
    gs.close()


def test_cli_denoised_animation(pkg, torch_cuda, tmp_path):
    cfg = json.load(open(os.path.join(ROOT, SCENE_FILES["cover"])))
    cfg.update(width=96, height=64, samples_per_pixel=8)
    path = tmp_path / "small.json"
    path.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    run = lambda args, env=None: subprocess.run([exe, str(path), *args], capture_output=True, text=True, cwd=ROOT, timeout=300, env=env)
    one, prefix = str(tmp_path / "one.png"), str(tmp_path / "anim")
    r1 = run([one, "--denoise"])
    r3 = run([prefix, "--frames", "3", "--orbit", "3", "--denoise"])
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr, r3.stderr)
    frames = [open(f"{prefix}_{f:03d}.png", "rb").read() for f in range(3)]
    assert frames[0] == open(one, "rb").read(), "frame 0 is not the --denoise one-shot PNG"
    assert len(set(frames)) == 3 and not os.path.exists(f"{prefix}_003.png")
    assert r3.stdout.count("\nRendering ") == 3 and r3.stdout.count("Frame time: ") == 3, r3.stdout
    r = run([str(tmp_path / "multi"), "--frames", "3", "--orbit", "3", "--denoise"], env=dict(os.environ, RT_GPUS="2"))
    assert r.returncode == 101 and len(r.stderr.strip().splitlines()) == 1 and "RT_GPUS" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "multi_000.png"))
