"""The device solid-texture code on adversarial points, bit for bit.

The contract of Checker and Noise spheres is "the bits of csrc/common/rt_solid.h".  tests/test_solid_cpu.py pins them for the host build
of that header against the restatement of tests/solid_mini.py; the device compiles the header with another compiler — its own expansion
of (uint32)(int32)(int64)floor(p), a target that has a `fract` beside x - floor(x) — and wraps it in a cold by-value call, rt_core.h
solid_albedo.  A frame reaches that code at some thousand ordinary hit points.  Here the point tables of tests/solid_points.py (the CPU
test's own) go through the device:
  - rt_hip_solid_fn_probe (librt_hip_probe.so): rt_solid_noise, rt_solid_noise_factor and rt_solid_checker_odd as f64 / parity, for every
    class, every seed and every (mode, octaves) of the class, in launches of 1 000 points (the last wave of each is partial).  Each must
    equal tests/lane_sim.py's solid_noise_v, solid_factor_v and solid_checker_v — the g++ build of the same header — bit for bit, the sign
    of a zero included.  With the CPU test this reads: device = host build = restatement;
  - rt_hip_solid_probe: rt_core.h solid_albedo on the records of a resident scene with one Checker and three Noise spheres: at centre 0
    and scale 1 the point is p itself, so every class goes through it; at another centre and scales 2.5 and 1/3, 10^4 points on and near
    each sphere.  The f32 colours must equal lane_sim's solid_albedo_v.
There is no tolerance anywhere.  That the tables reach the edges they are about is checked in numpy by the tests without the gpu mark."""
import ctypes as C
import functools

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import lane_sim
import solid_mini as SM
import solid_points as SP

CHUNK = 1000                                      # points per probe launch: 15 waves + 40 lanes, the last wave partial


@pytest.fixture(scope="module")
def sim(abi):
    return lane_sim.load(abi)


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _sim():
    from conftest import graft
    return lane_sim.load(graft.load_package().abi)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared tables are read-only)


@functools.lru_cache(maxsize=None)
def _fn_reference(cls, mode, octaves, seed):
    """the host build on the class's table: factor (as bits), noise (as bits), parity"""
    L, p = _sim(), SP.class_points(cls)
    with np.errstate(all="ignore"):
        return L.solid_factor_v(p, mode, octaves, seed).view(np.uint64), L.solid_noise_v(p, seed).view(np.uint64), L.solid_checker_v(p)


def _first(bad, p, got, want):
    i = np.flatnonzero(bad)[:3]
    return f"{int(bad.sum())} differ; first rows {i.tolist()}: points {p[i].tolist()} device {[hex(int(v)) for v in got[i]]} host {[hex(int(v)) for v in want[i]]}"


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", SP.CLASSES)
def test_device_solid_functions_equal_the_host_build(pkg, sim, torch_cuda, cls):
    """every (mode, octaves) of the class under every seed: the class's >= 10^5 points through rt_hip_solid_fn_probe in launches of 1 000,
    all three outputs at once; factor and noise in their 64 bits, the parity as it is"""
    L = pkg.hip.probe_lib()
    p = SP.class_points(cls)
    n = len(p)
    d_p = _dev(p)
    stream = torch.cuda.current_stream().cuda_stream
    for mode, octaves in SP.class_modes(cls):
        for seed in SP.SEEDS:
            d_factor = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
            d_noise = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
            d_odd = torch.full((n,), -2, dtype=torch.int32, device="cuda:0")
            for off in range(0, n, CHUNK):
                m = min(CHUNK, n - off)
                rc = L.rt_hip_solid_fn_probe(d_p.data_ptr() + 24 * off, mode, octaves, seed, d_noise.data_ptr() + 8 * off, d_factor.data_ptr() + 8 * off,
                                             d_odd.data_ptr() + 4 * off, m, stream)
                assert rc == 0, (rc, off)
            torch.cuda.synchronize()
            w_factor, w_noise, w_odd = _fn_reference(cls, mode, octaves, seed)
            g_factor, g_noise, g_odd = d_factor.cpu().numpy().view(np.uint64), d_noise.cpu().numpy().view(np.uint64), d_odd.cpu().numpy()
            what = f"{cls} mode {mode} octaves {octaves} seed {seed:#x}"
            assert np.array_equal(g_factor, w_factor), f"{what}: factor: " + _first(g_factor != w_factor, p, g_factor, w_factor)
            assert np.array_equal(g_noise, w_noise), f"{what}: noise: " + _first(g_noise != w_noise, p, g_noise, w_noise)
            assert np.array_equal(g_odd, w_odd), f"{what}: parity: " + _first(g_odd != w_odd, p, g_odd, w_odd)


@pytest.mark.gpu
def test_solid_fn_probe_outputs_are_optional_and_arguments_checked(pkg, abi, sim, torch_cuda):
    L = pkg.hip.probe_lib()
    p = SP.class_points("mixed")[:CHUNK]
    d_p = _dev(p)
    out = torch.full((CHUNK,), float("nan"), dtype=torch.float64, device="cuda:0")
    odd = torch.full((CHUNK,), -2, dtype=torch.int32, device="cuda:0")
    assert L.rt_hip_solid_fn_probe(d_p.data_ptr(), SM.MODE_MARBLE, 6, 3, None, out.data_ptr(), None, CHUNK, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), sim.solid_factor_v(p, SM.MODE_MARBLE, 6, 3).view(np.uint64)) and (odd.cpu().numpy() == -2).all()
    assert L.rt_hip_solid_fn_probe(d_p.data_ptr(), 0, 7, 0, None, None, odd.data_ptr(), CHUNK, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(odd.cpu().numpy(), sim.solid_checker_v(p))
    assert L.rt_hip_solid_fn_probe(d_p.data_ptr(), 0, 7, 0, None, None, None, 0, None) == 0
    for mode, octaves in ((3, 7), (0, 0), (1, 17)):
        assert L.rt_hip_solid_fn_probe(d_p.data_ptr(), mode, octaves, 0, None, out.data_ptr(), None, CHUNK, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_solid_fn_probe(None, 0, 7, 0, None, out.data_ptr(), None, CHUNK, None) == abi.RT_ERR_INVALID


# ------------------------------------------------------------------ solid_albedo on a resident scene's records
SOLIDS = [dict(kind="checker"), dict(kind="noise", mode=SM.MODE_NOISE, octaves=7, seed=0), dict(kind="noise", mode=SM.MODE_TURBULENCE, octaves=4, seed=0xFFFFFFFF),
          dict(kind="noise", mode=SM.MODE_MARBLE, octaves=6, seed=3)]
FAR_CENTRE = (13.25, -7.5, 101.125)


def _solid_scene(abi, centre, scales):
    """sphere 0 Lambertian, spheres 1 .. 4 the SOLIDS at `centre` (the same centre: solid_albedo knows no geometry but the centre), sphere
    k with scale scales[k - 1]; -> (scene, the array that keeps its spheres alive)"""
    arr = (abi.RtSphere * 5)()
    arr[0].center[:] = [0.0, -1000.0, 0.0]
    arr[0].radius, arr[0].kind = 10.0, abi.RT_MAT_LAMBERTIAN
    arr[0].albedo[:] = [0.5, 0.5, 0.5]
    for s, m, scale in zip(arr[1:], SOLIDS, scales):
        s.center[:] = list(centre)
        s.radius, s.h_offset = 2.0, scale
        s.albedo[:] = [0.9, 0.3, 0.7]
        if m["kind"] == "checker":
            s.kind = abi.RT_MAT_CHECKER
            s.tex_w, s.tex_h = abi.checker_odd_pack((0.125, 1.0, 0.3))
        else:
            s.kind, s.tex_id, s.tex_w, s.tex_h = abi.RT_MAT_NOISE, m["mode"], m["octaves"], m["seed"]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=1, max_depth=2, sky_mode=abi.RT_SKY_GRADIENT, spheres=arr,
                     n_spheres=5, seed=11)
    sc.cam_origin[:] = [0.0, 0.0, 30.0]
    sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]
    sc.cam_horizontal[:] = [3.0, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    return sc, arr


@functools.lru_cache(maxsize=None)
def _far_points():
    """10^4 points on and near the sphere of radius 2 at FAR_CENTRE: on it, a few ulps off it, and up to a radius inside and outside"""
    rng = np.random.default_rng(1750)
    d = rng.standard_normal((10_000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rad = np.where(rng.random(10_000) < 0.5, 2.0, 2.0 * rng.uniform(0.0, 2.0, 10_000))
    p = np.ascontiguousarray(np.array(FAR_CENTRE) + d * rad[:, None])
    p.setflags(write=False)
    return p


def _albedo_on_device(gs, sphere, points):
    n = len(points)
    d_p = _dev(points)
    d_rgb = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for off in range(0, n, CHUNK):
        gs.solid_probe(sphere, d_p.data_ptr() + 24 * off, d_rgb.data_ptr() + 12 * off, min(CHUNK, n - off), stream=stream)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", SP.CLASSES + ["far_centre"])
def test_device_solid_albedo_equals_the_host_build(pkg, abi, sim, torch_cuda, cls):
    """solid_albedo through rt_hip_solid_probe on the Checker sphere and the three Noise spheres (noise; turbulence, 4 octaves, seed 2^32 - 1;
    marble, 6 octaves) against lane_sim's solid_albedo_v, as 32-bit patterns.  The classes at centre 0 and scale 1 (p is the point);
    far_centre: centre (13.25, -7.5, 101.125), scales 2.5 and 1/3, 10^4 points on and near the sphere"""
    if cls == "far_centre":
        sc, keep = _solid_scene(abi, FAR_CENTRE, (2.5, 1.0 / 3.0, 2.5, 1.0 / 3.0))
        points = _far_points()
    else:
        sc, keep = _solid_scene(abi, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0))
        points = SP.class_points(cls)
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib())
    try:
        assert gs.query("solids") == 4
        for sphere in range(1, 5):
            rc, want = sim.solid_albedo_v(sc, sphere, points)
            assert rc == 0
            got = _albedo_on_device(gs, sphere, points)
            bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
            assert not bad.any(), (f"{cls} sphere {sphere}: {int(bad.sum())} colours differ; first rows {np.flatnonzero(bad)[:3].tolist()}: points "
                                   f"{points[np.flatnonzero(bad)[:3]].tolist()} device {got[bad][:3].tolist()} host {want[bad][:3].tolist()}")
            if cls in ("mixed", "far_centre"):
                assert len(np.unique(want, axis=0)) > (1 if sphere == 1 else 100), "the points do see the texture"
    finally:
        gs.close()


@pytest.mark.gpu
def test_solid_probe_refuses_other_spheres(pkg, abi, torch_cuda):
    sc, keep = _solid_scene(abi, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0))
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib())
    try:
        d_p = _dev(np.zeros((8, 3)))
        d_rgb = torch.zeros((8, 3), dtype=torch.float32, device="cuda:0")
        for sphere in (0, sc.n_spheres, 0xFFFFFFFF):        # a Lambertian sphere; an index equal to n_spheres; far outside
            with pytest.raises(pkg.host.RtError) as e:
                gs.solid_probe(sphere, d_p.data_ptr(), d_rgb.data_ptr(), 8)
            assert e.value.code == abi.RT_ERR_INVALID, sphere
        gs.solid_probe(1, d_p.data_ptr(), d_rgb.data_ptr(), 0)      # (no points: nothing is launched)
    finally:
        gs.close()
