"""Temporal denoising with surface tracking on the GPU (include/rt_abi.h rt_hip_render_surface / rt_hip_reproject_surface /
rt_hip_temporal_surface, the CLI's --temporal-surface).  Both kernels against tests/temporal_surface_ref.py (numpy,
written from the header's text) bit for bit; the host form against the public calls it is made of."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import temporal_cases as TC
import temporal_surface_cases as SC
import temporal_surface_ref as R

try:   # (before librt_hip.so is loaded, as collecting the whole suite does: the process then holds ONE HIP runtime, torch's)
    import torch  # noqa: F401
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = "scenes/cover_motion_1200x800_spp128.json"
FOG = "scenes/cover_fog_1200x800_spp128.json"
F = np.float32
GUARD = 0x7777777777777777
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


def _dev_surf(torch, s):
    return _dev(torch, np.ascontiguousarray(s, R.SURF).view(np.int64).reshape(s.shape + (2,)))


def _scene_cam(sc):
    return np.array(list(sc.c.cam_origin) + list(sc.c.cam_lower_left) + list(sc.c.cam_horizontal) + list(sc.c.cam_vertical), np.float64)


def _orbit_camera(host, path, deg):
    """the scene file's camera turned by deg about the y axis around look_at (the scenes' vup), as 12 doubles"""
    cam = json.load(open(os.path.join(ROOT, path)))["camera"]
    v = lambda k: np.array([cam[k]["x"], cam[k]["y"], cam[k]["z"]])
    d = host.camera_derive(list(TC.orbit(v("look_from"), v("look_at"), deg)), list(v("look_at")), list(v("vup")), cam["vfov"], cam["aspect"])
    return np.array(d["origin"] + d["lower_left_corner"] + d["horizontal"] + d["vertical"])


def _set_camera(gs, cam):
    gs.set_camera(list(cam[0:3]), list(cam[3:6]), list(cam[6:9]), list(cam[9:12]))


def _centres(sc):
    return np.array([[sc.c.spheres[i].center[k] for k in range(3)] for i in range(sc.c.n_spheres)], np.float64)


def _surface(torch, gs, as_device=False):
    """rt_hip_render_surface into a buffer with guard words on both sides -> the records [h, w] (and the device buffer)"""
    h, w = gs.height, gs.width
    buf = torch.full((h * w * 2 + 4,), GUARD, dtype=torch.int64, device="cuda:0")
    gs.render_surface(buf.data_ptr() + 16, stream=_stream(torch))
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[:2] == GUARD).all() and (g[-2:] == GUARD).all(), "words outside d_surface were written"
    rec = np.ascontiguousarray(g[2:-2]).view(R.SURF).reshape(h, w)
    return (rec, buf[2:-2]) if as_device else rec


def _aovs(torch, gs, n):
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(n, aov.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    return aov


def _linear(torch, gs, begin, count):
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    gs.accumulate(acc.data_ptr(), begin, count, stream=_stream(torch))
    gs.wait()
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), count, 0, lin.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    return lin


def _gpu_step(torch, gs, lin, aov, surf, prev_hist, prev_aov, prev_surf, prev_cam, disp, params):
    """rt_hip_reproject_surface into a buffer with guard words on both sides; params = alpha_min, alpha_specular, n_max, tau_n, tau_a, tau_z"""
    h, w = gs.height, gs.width
    guard = torch.full((h * w * 4 + 8,), -7.0, dtype=torch.float32, device="cuda:0")
    d = None if disp is None else _dev(torch, np.asarray(disp, np.float64))
    gs.reproject_surface(lin.data_ptr(), aov.data_ptr(), surf.data_ptr(), prev_hist.data_ptr(), prev_aov.data_ptr(), prev_surf.data_ptr(), prev_cam,
                         guard.data_ptr() + 16, d_displacement=0 if d is None else d.data_ptr(),
                         params=(params[0],) + tuple(params[2:]), alpha_specular=params[1], stream=_stream(torch))
    torch.cuda.synchronize()
    g = guard.cpu().numpy()
    assert (g[:4] == -7.0).all() and (g[-4:] == -7.0).all(), "words outside d_out_history were written"
    return g[4:-4].reshape(h, w, 4)


def _same_hist(got, want, what):
    bad = np.argwhere((_bits(got) != _bits(want)).any(-1))
    assert bad.size == 0, (what, len(bad), [(tuple(p), got[tuple(p)], want[tuple(p)]) for p in bad[:3]])


def _same_surf(got, want, what):
    bad = np.argwhere(got.view(np.uint64).reshape(got.shape + (2,)) != want.view(np.uint64).reshape(want.shape + (2,)))
    assert bad.size == 0, (what, len(bad), [(tuple(p[:2]), got[tuple(p[:2])], want[tuple(p[:2])]) for p in bad[:3]])


@pytest.mark.parametrize("name,w,h", [("cover", 96, 64), ("test", 96, 64), ("cover", 1, 9), ("cover", 9, 1), ("cover", 33, 17)])
def test_surface_matches_brute_force(pkg, torch_cuda, load_scene, name, w, h):
    sc = load_scene(name, w, h, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    got = _surface(torch_cuda, gs)
    gs.close()
    _same_surf(got, R.scene_surface(sc), (name, w, h))
    if w > 1 and h > 1:
        assert (got["id"] != R.NONE).mean() > 0.3 and (got["id"] == R.NONE).any()
    else:
        assert (got["id"] == R.NONE).all()      # (u or v divides by zero: the ray is not finite and hits nothing)


def test_surface_of_moving_spheres_is_at_half_the_shutter(pkg, torch_cuda, load_scene):
    sc = load_scene(MOTION, 96, 64, 4)
    c1 = np.array(sc.center1(), np.float64).reshape(-1, 3)
    gs = pkg.hip.HipScene(sc.ptr, 0, center1=c1)
    got = _surface(torch_cuda, gs)
    _same_surf(got, R.scene_surface(sc, center1=c1), "cover_motion")
    assert (got.view(np.uint64) != R.scene_surface(sc).view(np.uint64)).any(), "the moving spheres must show"
    moved = _centres(sc) + 0.25 * (c1 - _centres(sc))         # ... and after an update, of the tables it built
    gs.update_spheres(moved, c1)
    _same_surf(_surface(torch_cuda, gs), R.scene_surface(sc, center=moved, center1=c1), "cover_motion, updated")
    gs.close()


def test_surface_of_a_scene_above_65535_spheres(pkg, torch_cuda, host):
    """the wide tables (32-bit item lists), through test_more_than_65535_spheres' fixture"""
    from fuzz_worlds import big_flat_world_json
    sc = host.Scene.loads(big_flat_world_json(66000, np.random.default_rng(3), width=16, height=10))
    gs = pkg.hip.HipScene(sc.ptr, 0)
    assert gs.query("grid_wide") == 1
    got = _surface(torch_cuda, gs)
    gs.close()
    _same_surf(got, R.scene_surface(sc), "66001 spheres")
    assert (got["id"] != R.NONE).mean() > 0.5


def test_surface_of_the_fog_scene_follows_the_medium_candidate(pkg, torch_cuda, load_scene):
    """Checked against tests/medium_mini.py's hit_world — the candidate rule of DESIGN.md §15 restated from the contract, imported for this
    purpose — with the RNG address (this pixel, sample 0, node 0), at 32 x 20 (the restatement is plain Python)."""
    import medium_mini as MM
    sc = load_scene(FOG, 32, 20, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    assert gs.query("media") > 0
    got = _surface(torch_cuda, gs)
    gs.close()
    mm = MM.MediumMini(sc.c, math.atan2)
    cam = _scene_cam(sc)
    d = R.centre_rays(cam, 20, 32)
    o = tuple(float(x) for x in cam[0:3])
    want = np.zeros((20, 32), R.SURF)
    mm.sample = 0
    for y in range(20):
        for x in range(32):
            mm.pixel = y * 32 + x
            hit = mm.hit_world(o, tuple(float(v) for v in d[y, x]), 0)
            want[y, x] = (R.NONE, R.NONE, 0.0) if hit is None else (hit[0], sc.c.spheres[hit[0]].kind, mm.last_t)
    _same_surf(got, want, "fog")
    assert (got["kind"] == MM.MEDIUM).any() and ((got["kind"] != MM.MEDIUM) & (got["id"] != R.NONE)).any()


def test_surface_calls_leave_nothing_behind(pkg, torch_cuda, load_scene):
    """a plain frame and a progressive pass after surface records and a surface-mode frame are the ones made before any surface call"""
    sc = load_scene("cover", 96, 64, 6)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    plain, _ = gs.render_to_host()
    first, _ = gs.refine_to_host(3)
    _surface(torch_cuda, gs)
    gs.temporal_surface(True)
    for f in range(2):
        gs.render_frame_temporal_to_host(f, 2)
    assert np.array_equal(gs.render_to_host()[0], plain)
    assert gs.query("accum_samples") == 3
    second, _ = gs.refine_to_host(3)
    gs.close()
    fresh = pkg.hip.HipScene(sc.ptr, 0)
    assert np.array_equal(fresh.refine_to_host(6)[0], second) and np.array_equal(fresh.render_to_host()[0], plain)
    fresh.close()


@pytest.mark.parametrize("h,w", TC.SIZES)
def test_step_matches_numpy_on_crafted_frames(pkg, torch_cuda, load_scene, h, w):
    torch = torch_cuda
    rng = np.random.default_rng(1000 * h + w)
    lin, aov, prev_hist, prev_aov = TC.crafted(rng, h, w)
    surf, prev_surf = SC.crafted_surface(rng, aov, h, w)
    sc = load_scene("cover", w, h, 4)
    assert sc.c.n_spheres >= SC.N_IDS
    gs = pkg.hip.HipScene(sc.ptr, 0)
    d = [_dev(torch, lin), _dev(torch, aov), _dev_surf(torch, surf), _dev(torch, prev_hist), _dev(torch, prev_aov), _dev_surf(torch, prev_surf)]
    for dname, disp in SC.displacements(rng).items():
        full = None if disp is None else np.concatenate([disp, np.zeros((sc.c.n_spheres - SC.N_IDS, 3))])   # (the call reads n_spheres rows)
        for name, (cam, prev_cam) in TC.camera_pairs().items():
            _set_camera(gs, cam)
            for params in SC.PARAMS:
                got = _gpu_step(torch, gs, *d, prev_cam, full, params)
                want = R.reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, disp, *params)
                _same_hist(got, want, (h, w, dname, name, params))
    gs.close()


@pytest.mark.parametrize("name", ["cover", "test"])
def test_step_matches_numpy_on_real_frames(pkg, host, torch_cuda, load_scene, name):
    """8-spp colours, real guides and surface records at 96 x 64 over a 3 degree orbit: three frames, each against the one before"""
    torch = torch_cuda
    sc = load_scene(name, 96, 64, 8)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    cams = [_orbit_camera(host, TC_SCENES[name], 3.0 * f) for f in range(3)]
    for params in ((0.0, 1.0, 1e30, 0.1, 0.05, 0.1), (0.2, 0.5, 4.0, 1e30, 1e30, 1e30), (0.1, 0.0, 32.0, 0.0, 0.0, 0.0)):
        prev_hist = torch.zeros((64, 96, 4), dtype=torch.float32, device="cuda:0")
        prev_aov = torch.zeros((64, 96, 8), dtype=torch.float32, device="cuda:0")
        prev_surf = torch.zeros((64, 96, 2), dtype=torch.int64, device="cuda:0")
        prev_rec, prev_cam = np.zeros((64, 96), R.SURF), cams[0]
        reused = []
        for f, cam in enumerate(cams):
            _set_camera(gs, cam)
            lin, aov = _linear(torch, gs, 8 * f, 8), _aovs(torch, gs, 8)
            rec, surf = _surface(torch, gs, as_device=True)
            _same_surf(rec, R.scene_surface(sc, cam=cam), (name, f))
            got = _gpu_step(torch, gs, lin, aov, surf, prev_hist, prev_aov, prev_surf, prev_cam, None, params)
            want = R.reproject(lin.cpu().numpy(), aov.cpu().numpy(), rec, prev_hist.cpu().numpy(), prev_aov.cpu().numpy(), prev_rec, cam, prev_cam, None, *params)
            _same_hist(got, want, (name, params, f))
            reused.append(float((got[..., 3] > 1).mean()))
            prev_hist, prev_aov, prev_surf, prev_rec, prev_cam = _dev(torch, got), aov, surf.clone(), rec, cam
        print(name, params, "pixels with history per frame:", reused)
        assert reused[0] == 0.0, reused
        if params[3] > 0:
            assert reused[1] > 0.25 and reused[2] > 0.25, (name, params, reused)
    gs.close()


TC_SCENES = {"cover": "scenes/cfg2_cover_1200x800_spp128.json", "test": "scenes/cfg1_test_800x600_spp16.json"}


def _moving_frames(sc, n_frames, shutter=0.5):
    """the spheres of frame f of an animation along centre -> center1: (centre, center1) per frame"""
    c0 = _centres(sc)
    dv = np.array(sc.center1(), np.float64).reshape(-1, 3) - c0
    return [(c0 + dv * (f / n_frames), c0 + dv * ((f + shutter) / n_frames)) for f in range(n_frames)]


def test_step_matches_numpy_with_spheres_moved_between_frames(pkg, host, torch_cuda, load_scene):
    """three frames of cover_motion, rt_hip_scene_update_spheres between them, the displacement from the host arithmetic of the header:
    mid = c + (c1 - c) * 0.5 per frame, now - previous"""
    torch = torch_cuda
    sc = load_scene(MOTION, 96, 64, 8)
    frames = _moving_frames(sc, 3)
    gs = pkg.hip.HipScene(sc.ptr, 0, center1=frames[0][1])
    cam = _scene_cam(sc)
    params = (0.1, 1.0, 8.0, 0.1, 0.3, 0.05)
    prev_hist = torch.zeros((64, 96, 4), dtype=torch.float32, device="cuda:0")
    prev_aov = torch.zeros((64, 96, 8), dtype=torch.float32, device="cuda:0")
    prev_surf = torch.zeros((64, 96, 2), dtype=torch.int64, device="cuda:0")
    prev_rec, prev_mid = np.zeros((64, 96), R.SURF), None
    for f, (c, c1) in enumerate(frames):
        gs.update_spheres(c, c1)
        mid = R.mid_centres(c, c1)
        disp = np.zeros_like(mid) if prev_mid is None else mid - prev_mid
        lin, aov = _linear(torch, gs, 8 * f, 8), _aovs(torch, gs, 8)
        rec, surf = _surface(torch, gs, as_device=True)
        _same_surf(rec, R.scene_surface(sc, center=c, center1=c1), f)
        got = _gpu_step(torch, gs, lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, disp, params)
        want = R.reproject(lin.cpu().numpy(), aov.cpu().numpy(), rec, prev_hist.cpu().numpy(), prev_aov.cpu().numpy(), prev_rec, cam, cam, disp, *params)
        _same_hist(got, want, f)
        if f:
            still = _gpu_step(torch, gs, lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, None, params)
            assert (_bits(still) != _bits(got)).any(), "the displacement must matter"
        prev_hist, prev_aov, prev_surf, prev_rec, prev_mid = _dev(torch, got), aov, surf.clone(), rec, mid
    gs.close()


def test_a_moved_sphere_keeps_its_history(pkg, abi, torch_cuda, load_scene):
    """The cover's big Lambertian sphere moved by its radius between two frames, thresholds 1e30, a static camera.  The pixels are chosen
    by the numpy reference: those whose four taps all lie on the sphere's previous footprint.  With the displacement each has n = 2;
    with none, the taps stay where the pixel is and those outside the old footprint start over."""
    torch = torch_cuda
    sc = load_scene("cover", 96, 64, 4)
    n = sc.c.n_spheres
    c0 = _centres(sc)
    big = [i for i in range(n) if sc.c.spheres[i].kind == abi.RT_MAT_LAMBERTIAN and sc.c.spheres[i].radius == 1.0]
    assert len(big) == 1
    i = big[0]
    c1 = c0.copy()
    c1[i] += (0.0, 0.0, 1.0)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    cam = _scene_cam(sc)
    params = (0.0, 0.0, 1e30, 1e30, 1e30, 1e30)
    zero_h = torch.zeros((64, 96, 4), dtype=torch.float32, device="cuda:0")
    zero_a = torch.zeros((64, 96, 8), dtype=torch.float32, device="cuda:0")
    zero_s = torch.zeros((64, 96, 2), dtype=torch.int64, device="cuda:0")
    lin0, aov0 = _linear(torch, gs, 0, 4), _aovs(torch, gs, 4)
    rec0, surf0 = _surface(torch, gs, as_device=True)
    hist0 = _gpu_step(torch, gs, lin0, aov0, surf0, zero_h, zero_a, zero_s, cam, None, params)
    assert (hist0[..., 3] == 1.0).all() and not np.isnan(hist0).any()
    gs.update_spheres(c1)
    lin1, aov1 = _linear(torch, gs, 4, 4), _aovs(torch, gs, 4)
    assert not np.isnan(lin1.cpu().numpy()).any()
    rec1, surf1 = _surface(torch, gs, as_device=True)
    disp = c1 - c0
    ok, same = R.taps(rec1, rec0, cam, cam, disp)
    chosen = ok & (rec1["id"] == i) & same[0] & same[1] & same[2] & same[3]
    assert chosen.sum() >= 20, int(chosen.sum())
    with_d = _gpu_step(torch, gs, lin1, aov1, surf1, _dev(torch, hist0), aov0, surf0, cam, disp, params)
    without = _gpu_step(torch, gs, lin1, aov1, surf1, _dev(torch, hist0), aov0, surf0, cam, None, params)
    gs.close()
    print(f"{int(chosen.sum())} pixels of the moved sphere; with no displacement {int((without[chosen][:, 3] == 2.0).sum())} of them keep history")
    assert (with_d[chosen][:, 3] == 2.0).all(), np.unique(with_d[chosen][:, 3], return_counts=True)
    assert not (without[chosen][:, 3] == 2.0).all()


def test_specular_floor_and_running_mean(pkg, abi, torch_cuda, load_scene):
    """Static camera, four frames of 4 spp through the host form, alpha_min 0, alpha_specular 1, no cap on n.  A Metal or Glass pixel holds
    this frame's colour c to the roundings of out = hist + 1 (c - hist): two f32 operations, |out - c| <= 2^-24 (2 |c| + |hist|) (1 + 2^-20)
    with |hist| at most the largest value of the previous history.  Every other pixel holds the mean of samples [0, 16) within
    test_static_camera_accumulates_the_running_mean's bound for four frames: 4 * 4 * 2^-24 * max(1, value)."""
    torch = torch_cuda
    sc = load_scene("cover", 96, 64, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.temporal_configure(0.0, 1e30, 0.1, 0.1, 0.1)
    gs.temporal_surface(True, 1.0)
    for f in range(3):
        gs.render_frame_temporal_to_host(f, 0)
    before = gs.temporal_history()
    gs.render_frame_temporal_to_host(3, 0)
    hist = gs.temporal_history()
    rec = _surface(torch, gs)
    c = _linear(torch, gs, 12, 4).cpu().numpy().astype(np.float64)
    mean = _linear(torch, gs, 0, 16).cpu().numpy().astype(np.float64)
    gs.close()
    assert not np.isnan(c).any() and not np.isnan(mean).any()
    specular = (rec["kind"] == abi.RT_MAT_METAL) | (rec["kind"] == abi.RT_MAT_GLASS)
    assert specular.sum() > 200 and (~specular).sum() > 2000
    err_s = np.abs(hist[..., 0:3].astype(np.float64) - c)[specular]
    bound_s = (2.0 ** -24 * (2.0 * np.abs(c) + float(before[..., 0:3].max())) * (1.0 + 2.0 ** -20))[specular]
    print(f"specular pixels: max |history - this frame| {err_s.max():.3e}, max of err / bound {float((err_s / bound_s).max()):.3f}")
    assert (err_s <= bound_s).all(), (float(err_s.max()), int((err_s > bound_s).sum()))
    err_d = np.abs(hist[..., 0:3].astype(np.float64) - mean)[~specular]
    bound_d = (4 * 4 * 2.0 ** -24 * np.maximum(1.0, mean))[~specular]
    print(f"other pixels: max |history - mean of 16 samples| {err_d.max():.3e}, max of err / bound {float((err_d / bound_d).max()):.3f}")
    assert (hist[..., 3][~specular] == 4.0).all(), np.unique(hist[..., 3][~specular], return_counts=True)
    assert (err_d <= bound_d).all(), (float(err_d.max()), int((err_d > bound_d).sum()))


def test_host_form_is_the_six_public_calls(pkg, host, torch_cuda, load_scene):
    """three frames with an orbit and moved spheres: accumulate, resolve, AOVs, surface, reproject_surface, denoise composed here, against
    rt_hip_render_frame_temporal_to_host in surface mode, byte for byte in RGB8 and history; frame 0 is rt_hip_refine_to_host_denoised's"""
    torch = torch_cuda
    spp, its = 8, 2
    sc = load_scene(MOTION, 96, 64, spp)
    frames = _moving_frames(sc, 3)
    cams = [_orbit_camera(host, MOTION, 3.0 * f) for f in range(3)]
    k = (0.1, 6.0, 0.05, 0.3, 0.05)
    a_spec = 0.75
    form = pkg.hip.HipScene(sc.ptr, 0, center1=frames[0][1])
    form.temporal_configure(*k)
    assert form.query("temporal_surface") == 0
    form.temporal_surface(True, a_spec)
    assert form.query("temporal_surface") == 1
    mine = pkg.hip.HipScene(sc.ptr, 0, center1=frames[0][1])
    shape = (64, 96)
    prev_hist = torch.zeros(shape + (4,), dtype=torch.float32, device="cuda:0")
    prev_aov = torch.zeros(shape + (8,), dtype=torch.float32, device="cuda:0")
    prev_surf = torch.zeros(shape + (2,), dtype=torch.int64, device="cuda:0")
    prev_cam, prev_mid = cams[0], None
    for f, ((c, c1), cam) in enumerate(zip(frames, cams)):
        for gs in (form, mine):
            _set_camera(gs, cam)
            if f:
                gs.update_spheres(c, c1)
        want_rgb, _ = form.render_frame_temporal_to_host(f, its)
        want_hist = form.temporal_history()
        mid = R.mid_centres(c, c1)
        disp = _dev(torch, np.zeros_like(mid) if prev_mid is None else mid - prev_mid)
        lin, aov = _linear(torch, mine, spp * f, spp), _aovs(torch, mine, spp)
        _, surf = _surface(torch, mine, as_device=True)
        hist = torch.zeros(shape + (4,), dtype=torch.float32, device="cuda:0")
        mine.reproject_surface(lin.data_ptr(), aov.data_ptr(), surf.data_ptr(), prev_hist.data_ptr(), prev_aov.data_ptr(), prev_surf.data_ptr(), prev_cam,
                               hist.data_ptr(), d_displacement=disp.data_ptr(), params=k, alpha_specular=a_spec, stream=_stream(torch))
        rgb_in = hist[..., 0:3].contiguous()
        rgb8 = torch.zeros(shape + (3,), dtype=torch.uint8, device="cuda:0")
        mine.denoise(rgb_in.data_ptr(), aov.data_ptr(), its, 0, rgb8.data_ptr(), stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(hist.cpu().numpy()), _bits(want_hist)), f
        assert np.array_equal(rgb8.cpu().numpy(), want_rgb), f
        if f == 0:
            ref = pkg.hip.HipScene(sc.ptr, 0, center1=frames[0][1])
            _set_camera(ref, cam)
            assert np.array_equal(ref.refine_to_host_denoised(spp, its)[0], want_rgb), "frame 0 is not the denoised one-shot frame"
            ref.close()
        else:
            assert (want_hist[..., 3] > 1).mean() > 0.25
        prev_hist, prev_aov, prev_surf, prev_cam, prev_mid = hist, aov, surf.clone(), cam, mid
    # a change of mode drops the history; the same mode again keeps it
    form.temporal_surface(True, 0.5)
    form.temporal_history()
    form.temporal_surface(False, 0.5)
    assert form.query("temporal_surface") == 0
    with pytest.raises(pkg.host.RtError):
        form.temporal_history()
    form.close()
    mine.close()


def test_mode_off_is_the_path_without_surface_tracking(pkg, host, torch_cuda, load_scene):
    """enable 0 — after having been on, too — gives the bytes of a scene that never heard of rt_hip_temporal_surface"""
    sc = load_scene("cover", 96, 64, 8)
    cams = [_orbit_camera(host, TC_SCENES["cover"], 3.0 * f) for f in range(3)]
    plain, off = pkg.hip.HipScene(sc.ptr, 0), pkg.hip.HipScene(sc.ptr, 0)
    off.temporal_surface(True, 0.3)
    _set_camera(off, cams[0])
    off.render_frame_temporal_to_host(0, 2)
    off.temporal_surface(False, 0.3)
    for f, cam in enumerate(cams):
        _set_camera(plain, cam)
        _set_camera(off, cam)
        a, b = plain.render_frame_temporal_to_host(f, 2)[0], off.render_frame_temporal_to_host(f, 2)[0]
        assert np.array_equal(a, b), f
        assert np.array_equal(_bits(plain.temporal_history()), _bits(off.temporal_history())), f
    plain.close()
    off.close()


def test_surface_calls_refuse_bad_arguments_on_a_scene(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    h, w = 24, 32
    sc = load_scene("cover", w, h, 4)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    n = sc.c.n_spheres
    lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    aov, paov = (torch.zeros((h, w, 8), dtype=torch.float32, device="cuda:0") for _ in range(2))
    surf, psurf = (torch.zeros((h * w * 2 + 2,), dtype=torch.int64, device="cuda:0") for _ in range(2))
    hist = torch.zeros((h * w * 4 + 8,), dtype=torch.float32, device="cuda:0")
    out = torch.full((max(h * w * 4, n * 6) + 8,), 7.0, dtype=torch.float32, device="cuda:0")
    disp = torch.zeros((n * 3 + 1,), dtype=torch.float64, device="cuda:0")
    L, s = pkg.hip.lib(), gs._h
    cam = (C.c_double * 12)(*TC.camera_pairs()["identical"][0])
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    good = (0.1, 1.0, 32.0, 0.1, 0.1, 0.1)

    def call(lin_=p(lin), aov_=p(aov), surf_=p(surf), hist_=p(hist), paov_=p(paov), psurf_=p(psurf), cam_=cam, disp_=p(disp), k=good, out_=p(out)):
        return L.rt_hip_reproject_surface(s, lin_, aov_, surf_, hist_, paov_, psurf_, cam_, disp_, *k, out_, None)
    cases = [call(lin_=None), call(aov_=None), call(surf_=None), call(hist_=None), call(paov_=None), call(psurf_=None), call(cam_=None), call(out_=None),
             call(lin_=p(lin, 2)), call(aov_=p(aov, 4)), call(surf_=p(surf, 8)), call(hist_=p(hist, 8)), call(paov_=p(paov, 4)), call(psurf_=p(psurf, 8)),
             call(disp_=p(disp, 4)), call(out_=p(out, 8)),
             call(out_=p(hist)), call(out_=p(hist, 16)), call(out_=p(lin)), call(out_=p(aov)), call(out_=p(paov)), call(out_=p(surf)), call(out_=p(psurf, 16)),
             call(disp_=p(out)), call(disp_=p(out, 8))]      # overlaps
    for i in range(3, 6):
        for bad in (-1.0, float("nan"), float("inf")):
            cases.append(call(k=good[:i] + (bad,) + good[i + 1:]))
    for i in (0, 1):
        for bad in (-0.01, 1.01, float("nan")):
            cases.append(call(k=good[:i] + (bad,) + good[i + 1:]))
    for bad in (0.5, 0.0, -1.0, float("nan")):
        cases.append(call(k=good[:2] + (bad,) + good[3:]))
    cases += [L.rt_hip_temporal_surface(s, 1, bad) for bad in (-0.01, 1.01, float("nan"))]
    cases += [L.rt_hip_render_surface(s, None, None, None), L.rt_hip_render_surface(s, None, p(out, 8), None)]
    for i, rc in enumerate(cases):
        assert rc == abi.RT_ERR_INVALID, (i, rc)
    assert gs.query("temporal_surface") == 0
    tiles = abi.RtRowTiles(2, 0, 2)
    assert L.rt_hip_render_surface(s, C.byref(tiles), p(out), None) == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all(), "a refused call wrote its output"
    assert call() == abi.RT_OK and call(disp_=None) == abi.RT_OK and call(k=(0.0, 0.0, float("inf"), 0.0, 0.0, 0.0)) == abi.RT_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[: h * w * 4] != 7.0).all()
    gs.close()


def _cli_orbit_camera(host, cam, deg, f):
    """main.cpp's orbit_camera: look_from turned about vup around look_at by deg * f (Rodrigues), the operations in its order"""
    v3 = lambda k: [cam[k]["x"], cam[k]["y"], cam[k]["z"]]
    lf, la, up = v3("look_from"), v3("look_at"), v3("vup")
    kl = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    k = [up[i] / kl for i in range(3)]
    th = deg * f * (3.14159265358979323846264338327950288 / 180.0)
    c, s = math.cos(th), math.sin(th)
    v = [lf[i] - la[i] for i in range(3)]
    kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
    kx = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    frm = [la[i] + v[i] * c + kx[i] * s + k[i] * kv * (1.0 - c) for i in range(3)]
    d = host.camera_derive(frm, la, up, cam["vfov"], cam["aspect"])
    return np.array(d["origin"] + d["lower_left_corner"] + d["horizontal"] + d["vertical"])


def test_cli_surface_animation(pkg, host, torch_cuda, tmp_path):
    """--frames 3 --orbit 3 --denoise --temporal-surface writes the host form's three frames (configured with RT_TEMPORAL_SURFACE_*)"""
    from PIL import Image
    cfg = json.load(open(os.path.join(ROOT, TC_SCENES["cover"])))
    cfg.update(width=96, height=64, samples_per_pixel=8)
    path = tmp_path / "small.json"
    path.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    prefix = str(tmp_path / "anim")
    r = subprocess.run([exe, str(path), prefix, "--frames", "3", "--orbit", "3", "--denoise", "--temporal-surface"], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("\nRendering ") == 3 and not os.path.exists(f"{prefix}_003.png")
    sc = host.Scene.load(str(path))
    gs = pkg.hip.HipScene(sc.ptr, 0)
    a_min, a_spec = pkg.hip.HipScene.TEMPORAL_SURFACE_PARAMS
    gs.temporal_configure(a_min, *pkg.hip.HipScene.TEMPORAL_PARAMS[1:])
    gs.temporal_surface(True, a_spec)
    frames = []
    for f in range(3):
        _set_camera(gs, _cli_orbit_camera(host, cfg["camera"], 3.0, f))
        want, _ = gs.render_frame_temporal_to_host(f, pkg.hip.HipScene.DENOISE_ITERATIONS)
        got = np.asarray(Image.open(f"{prefix}_{f:03d}.png").convert("RGB"))
        assert np.array_equal(got, want), f
        frames.append(want)
    gs.close()
    assert not np.array_equal(frames[0], frames[1])
    # ... and they are not the frames of the mode without surface tracking
    r = subprocess.run([exe, str(path), str(tmp_path / "plain"), "--frames", "3", "--orbit", "3", "--denoise"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not np.array_equal(np.asarray(Image.open(str(tmp_path / "plain_002.png")).convert("RGB")), frames[2])
