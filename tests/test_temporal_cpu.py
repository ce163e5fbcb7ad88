"""Temporal denoising without a GPU (include/rt_abi.h rt_hip_reproject): the CPU build of rt_core.h's reproject_pixel
against tests/temporal_ref.py (numpy, written from the header's text) bit for bit; the pixel convention against analytic geometry;
the CLI's argument table; the new calls' declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_cases as TC
import temporal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
NEW = ("rt_hip_reproject", "rt_hip_render_frame_temporal_to_host", "rt_hip_temporal_configure", "rt_hip_temporal_reset", "rt_hip_temporal_history")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def reproject_step(tmp_path_factory):
    """CPU build of rt_core.h's reprojection step (tests/temporal/reproject_step.cpp), -ffp-contract=off"""
    so = str(tmp_path_factory.mktemp("reproject_step") / "libreproject_step.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared",
                    os.path.join(ROOT, "tests", "temporal", "reproject_step.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.reproject_step_frame.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.reproject_step_frame.restype = None

    def run(lin, aov, prev_hist, prev_aov, cam, prev_cam, params):
        h, w, _ = lin.shape
        bufs = [np.ascontiguousarray(a, np.float32) for a in (lin, aov, prev_hist, prev_aov)]
        cams = [np.ascontiguousarray(c, np.float64) for c in (cam, prev_cam)]
        k = np.array(params, np.float32)
        out = np.full((h, w, 4), -7.0, np.float32)
        L.reproject_step_frame(*[b.ctypes.data for b in bufs], *[c.ctypes.data for c in cams], w, h, k.ctypes.data, out.ctypes.data)
        return out
    return run


def test_temporal_calls_are_declared_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    for lib in (pkg.hip.LIB_PATH, pkg.hip.PROBE_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if l.split()}
        for n in NEW:
            assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} not declared in rt_abi.h"
            assert n in exported, f"{n} not exported by {os.path.basename(lib)}"
    shim = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert "fn " + n + "(" in shim, f"{n} missing from the Rust shim of INTEGRATION.md"
    for name in ("RT_TEMPORAL_ALPHA_MIN", "RT_TEMPORAL_N_MAX", "RT_TEMPORAL_TAU_NORMAL", "RT_TEMPORAL_TAU_ALBEDO", "RT_TEMPORAL_TAU_INV_DEPTH"):
        assert re.search(r"#define\s+" + name + r"\s", text), name


def test_python_defaults_are_the_headers(pkg):
    """HipScene.TEMPORAL_PARAMS restates include/rt_abi.h's RT_TEMPORAL_* (tools/temporal_bench.py reads it as the library's defaults)"""
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    names = ("RT_TEMPORAL_ALPHA_MIN", "RT_TEMPORAL_N_MAX", "RT_TEMPORAL_TAU_NORMAL", "RT_TEMPORAL_TAU_ALBEDO", "RT_TEMPORAL_TAU_INV_DEPTH")
    header = tuple(float(re.search(r"#define\s+" + n + r"\s+([0-9.eE+-]+)f\b", text).group(1)) for n in names)
    assert header == tuple(pkg.hip.HipScene.TEMPORAL_PARAMS), (header, pkg.hip.HipScene.TEMPORAL_PARAMS)


def test_temporal_calls_refuse_null_arguments(pkg, abi):
    L = pkg.hip.lib()
    p = C.c_void_p(64)   # (never dereferenced: every call below is refused before it looks at a buffer)
    cam = (C.c_double * 12)()
    assert L.rt_hip_reproject(None, p, p, p, p, cam, 0.1, 32.0, 0.1, 0.1, 0.1, p, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_render_frame_temporal_to_host(None, 0, 2, None, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_temporal_configure(None, 0.1, 32.0, 0.1, 0.1, 0.1) == abi.RT_ERR_INVALID
    assert L.rt_hip_temporal_reset(None) == abi.RT_ERR_INVALID
    assert L.rt_hip_temporal_history(None, None) == abi.RT_ERR_INVALID


@pytest.mark.parametrize("h,w", TC.SIZES)
def test_cpu_step_matches_numpy(reproject_step, h, w):
    rng = np.random.default_rng(1000 * h + w)
    lin, aov, prev_hist, prev_aov = TC.crafted(rng, h, w)
    seen_history = seen_none = False
    for name, (cam, prev_cam) in TC.camera_pairs().items():
        for params in TC.PARAMS:
            got = reproject_step(lin, aov, prev_hist, prev_aov, cam, prev_cam, params)
            want = temporal_ref.reproject(lin, aov, prev_hist, prev_aov, cam, prev_cam, *params)
            bad = np.argwhere((_bits(got) != _bits(want)).any(-1))
            assert bad.size == 0, (h, w, name, params, len(bad), [(tuple(p), got[tuple(p)], want[tuple(p)]) for p in bad[:3]])
            nan_px = np.isnan(lin).any(-1)
            assert np.array_equal(_bits(got[nan_px][:, :3]), _bits(lin[nan_px])) and (got[nan_px][:, 3] == 0).all(), "a NaN pixel: out = c, n = 0"
            assert not np.isnan(got[~nan_px]).any(), (h, w, name, params, "a NaN was written")
            n = got[~nan_px][:, 3]
            assert ((n >= 1) & (n <= F(params[1]))).all()
            fresh = n == 1
            assert np.array_equal(_bits(got[~nan_px][fresh][:, :3]), _bits(lin[~nan_px][fresh]))
            # (a < 0; w - 1 = 0 or h - 1 = 0; after a 90 degree jump the sky is off screen and no surface has bit-equal guides)
            if name == "behind" or h == 1 or w == 1 or (name == "orbit90" and params[2:] == (0.0, 0.0, 0.0)):
                assert fresh.all(), (h, w, name, params)
            if name == "identical" and params[2] > 1e29 and h > 1 and w > 1:
                seen_history = seen_history or (n > 1).any()
            if params[0] == 1.0:    # alpha_min = 1: the frame's own colour wherever history was found, whatever it held
                assert np.allclose(got[~nan_px][:, :3], lin[~nan_px], rtol=0, atol=2e-7)
            seen_none = seen_none or fresh.any()
    assert seen_none and (seen_history or h == 1 or w == 1)


def test_cases_reach_every_branch(reproject_step):
    """the crafted buffers are worth their name: with huge thresholds an identical camera finds history for most pixels, a 3 degree
    orbit and the camera in the middle of the scene for some; zero thresholds keep the taps whose guides are bit-equal only"""
    rng = np.random.default_rng(7)
    lin, aov, prev_hist, prev_aov = TC.crafted(rng, 32, 48)
    pairs = TC.camera_pairs()
    huge, zero = TC.PARAMS[0], TC.PARAMS[3]
    frac = {}
    for name, (cam, prev_cam) in pairs.items():
        frac[name] = float((reproject_step(lin, aov, prev_hist, prev_aov, cam, prev_cam, huge)[..., 3] > 1).mean())
    assert frac["identical"] > 0.7 and 0.2 < frac["orbit3"] < frac["identical"] and 0.0 < frac["through"] < 0.9, frac
    assert frac["behind"] == 0.0 and 0.0 < frac["orbit90"] < frac["identical"], frac   # (the points near look_at stay in view after a 90 degree jump)
    assert not (reproject_step(lin, aov, prev_hist, prev_aov, *pairs["orbit90"], zero)[..., 3] > 1).any()
    z = float((reproject_step(lin, aov, prev_hist, prev_aov, *pairs["identical"], zero)[..., 3] > 1).mean())
    assert 0.0 < z < frac["identical"], (z, frac)
    n = reproject_step(lin, aov, prev_hist, prev_aov, *pairs["identical"], (0.0, 3.0, 1e30, 1e30, 1e30))[..., 3]
    assert n.max() == 3.0 and (n == 3.0).sum() > 100, "n_max must cap the count"


def _first_hits(cam, h, w):
    """the pixel-centre rays of `cam` against the plane y = 0 and the sphere of radius 1 at (0, 1, 0): position [h, w, 3] (NaN: sky)
    and the AOV record [h, w, 8]"""
    org, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = (xs + 0.5) / (w - 1), (h - (ys + 0.5)) / (h - 1)
    d = ll + hor * u[..., None] + ver * v[..., None] - org
    with np.errstate(all="ignore"):
        t_plane = np.where(d[..., 1] < 0, -org[1] / d[..., 1], np.inf)
        c = np.array([0.0, 1.0, 0.0])
        oc = org - c
        a, hb, cc = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - 1.0
        disc = hb * hb - a * cc
        t_sph = np.where(disc >= 0, (-hb - np.sqrt(np.abs(disc))) / a, np.inf)
    t = np.minimum(t_plane, t_sph)
    hit = np.isfinite(t)
    pos = org + d * np.where(hit, t, 0.0)[..., None]
    pos[~hit] = np.nan
    aov = np.zeros((h, w, 8), F)
    on_sphere = hit & (t_sph < t_plane)
    aov[hit & ~on_sphere, 0:3] = (0.5, 0.5, 0.5)
    aov[hit & ~on_sphere, 4:7] = (0.0, 1.0, 0.0)
    aov[on_sphere, 0:3] = (0.9, 0.2, 0.1)
    aov[on_sphere, 4:7] = (pos - c)[on_sphere]
    aov[hit, 3] = (1.0 / t[hit]).astype(F)
    aov[hit, 7] = 1.0
    return pos, aov


def test_pixel_convention_against_analytic_geometry(reproject_step):
    """Two cameras 3 degrees apart over a plane and a sphere.  The previous frame's history holds the world position of its first hit;
    reprojected into the current camera it must land on the current camera's own positions — closer than the same history shifted by
    one pixel in any direction, which is what a missing half-pixel offset or a flipped v would amount to."""
    h, w = 64, 96
    la = np.array([0.0, 0.5, 0.0])
    lf = np.array([8.0, 3.0, 3.0])
    cur, prev = TC.camera(lf, la, vfov=30.0), TC.camera(TC.orbit(lf, la, -3.0), la, vfov=30.0)
    pos_cur, aov = _first_hits(cur, h, w)
    pos_prev, prev_aov = _first_hits(prev, h, w)
    hist = np.zeros((h, w, 4), F)
    hist[..., 0:3] = np.nan_to_num(pos_prev, nan=0.0)
    hist[..., 3] = 1.0
    lin = np.zeros((h, w, 3), F)   # c = 0, n' = 1, alpha_min = 0: out = hist / 2 exactly where history was found
    params = (0.0, 1e30, 0.05, 0.01, 0.05)   # (a sphere's normal turns by up to 0.1 across one pixel here)

    def median_error(hs):
        out = reproject_step(lin, aov, hs, prev_aov, cur, prev, params)
        ok = (out[..., 3] == 2.0) & (aov[..., 7] > 0)
        assert ok.mean() > 0.4, ok.mean()
        err = np.linalg.norm(2.0 * out[..., 0:3].astype(np.float64) - pos_cur, axis=-1)[ok]
        return float(np.median(err)), ok
    base, ok = median_error(hist)
    print(f"median reprojection error {base:.3e} over {int(ok.sum())} accepted pixels")
    assert (aov[ok][:, 0] > 0.8).any() and (aov[ok][:, 0] < 0.6).any(), "both the sphere and the plane must be among the accepted pixels"
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        shifted, _ = median_error(np.roll(hist, (dy, dx), axis=(0, 1)))
        print(f"  history shifted by ({dy}, {dx}): {shifted:.3e}")
        assert base < shifted, (dy, dx, base, shifted)


@pytest.mark.parametrize("args, usage", [
    (["--frames", "3", "--orbit", "3", "--denoise"], False),                        # the denoised animation
    (["--denoise", "--orbit", "0", "--frames", "3"], False),                        # ... a camera that stays
    (["--frames", "3", "--orbit", "3", "--shutter", "0.5", "--denoise"], False),     # ... with spheres moving from frame to frame
    (["--frames", "3", "--denoise"], True),                                         # the turn per frame must be named
    (["--frames", "3", "--shutter", "0.5", "--denoise"], True),
    (["--denoise", "--orbit", "10"], True),                                         # only with --frames
    (["--frames", "0", "--orbit", "3", "--denoise"], True),
    (["--frames", "3", "--orbit", "3", "--denoise", "--adaptive", "0.1"], True),
    (["--adaptive", "0.1", "--denoise"], True),
    (["--frames", "3", "--orbit", "3", "--denoise", "--passes", "2"], True),
    (["--denoise"], False),                                                         # the modes there were stay
    (["--passes", "4", "--denoise"], False),
    (["--frames", "3", "--orbit", "3"], False),
])
def test_cli_argument_table(pkg, tmp_path, args, usage):
    """a refused command line prints the usage line and returns 0 (main.rs:9-12) before anything is read; an accepted one goes on to
    read the scene file — which does not exist here"""
    r = subprocess.run([EXE, str(tmp_path / "missing.json"), str(tmp_path / "out")] + args, capture_output=True, text=True, timeout=60)
    if usage:
        assert r.returncode == 0 and r.stdout.startswith("Usage:"), (args, r.returncode, r.stdout, r.stderr)
    else:
        assert r.returncode == 101 and "Unable to read config file" in r.stderr and "Usage" not in r.stdout, (args, r.returncode, r.stdout, r.stderr)


def test_cli_refuses_several_gpus(pkg, tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "scenes/cfg1_test_800x600_spp16.json", out, "--frames", "3", "--orbit", "3", "--denoise"], capture_output=True, text=True,
                       cwd=ROOT, timeout=300, env=dict(os.environ, RT_GPUS="2"))
    assert r.returncode == 101 and len(r.stderr.strip().splitlines()) == 1 and "RT_GPUS" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out + "_000.png")
