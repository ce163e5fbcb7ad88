"""Temporal denoising with surface tracking, without a GPU (include/rt_abi.h rt_hip_render_surface / rt_hip_reproject_surface /
rt_hip_temporal_surface): the CPU builds of rt_core.h's surface_pixel and reproject_surface_pixel against
tests/temporal_surface_ref.py (numpy, written from the header's text) bit for bit; the motion vector against analytic geometry; the
new calls' declarations; the CLI's argument table."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lane_sim
import temporal_cases as TC
import temporal_surface_cases as SC
import temporal_surface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
NEW = ("rt_hip_render_surface", "rt_hip_reproject_surface", "rt_hip_temporal_surface")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def step(tmp_path_factory, abi):
    """CPU builds, -ffp-contract=off: reproject_surface_pixel in tests/temporal_surface/step.cpp, surface_pixel in tests/lanesim"""
    so = str(tmp_path_factory.mktemp("temporal_surface") / "libsurface_step.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared",
                    os.path.join(ROOT, "tests", "temporal_surface", "step.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.surface_step_frame.argtypes = [C.c_void_p] * 9 + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p]
    L.surface_step_frame.restype = None
    sim = lane_sim.load(abi)

    class Step:
        @staticmethod
        def reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, disp, params):
            h, w, _ = lin.shape
            f = [np.ascontiguousarray(a, np.float32) for a in (lin, aov, prev_hist, prev_aov)]
            s = [np.ascontiguousarray(a, R.SURF) for a in (surf, prev_surf)]
            cams = [np.ascontiguousarray(c, np.float64) for c in (cam, prev_cam)]
            d = None if disp is None else np.ascontiguousarray(disp, np.float64)
            k = np.array(params, np.float32)
            out = np.full((h, w, 4), -7.0, np.float32)
            L.surface_step_frame(f[0].ctypes.data, f[1].ctypes.data, s[0].ctypes.data, f[2].ctypes.data, f[3].ctypes.data, s[1].ctypes.data,
                                 cams[0].ctypes.data, cams[1].ctypes.data, None if d is None else d.ctypes.data, 0 if d is None else len(d), w, h,
                                 k.ctypes.data, out.ctypes.data)
            return out

        @staticmethod
        def surface(sc, center1=None):
            rc, out = sim.surface(sc.ptr, center1)
            assert rc == 0 and out.dtype == R.SURF
            return out
    return Step


def _same_hist(got, want, what):
    bad = np.argwhere((_bits(got) != _bits(want)).any(-1))
    assert bad.size == 0, (what, len(bad), [(tuple(p), got[tuple(p)], want[tuple(p)]) for p in bad[:3]])


def _same_surf(got, want, what):
    bad = np.argwhere(got.view(np.uint64).reshape(got.shape + (2,)) != want.view(np.uint64).reshape(want.shape + (2,)))
    assert bad.size == 0, (what, len(bad), [(tuple(p[:2]), got[tuple(p[:2])], want[tuple(p[:2])]) for p in bad[:3]])


def test_surface_calls_are_declared_and_exported(pkg):
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
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5u?\b", open(os.path.join(ROOT, "include", "rt_abi.h")).read())


def test_python_defaults_are_the_headers(pkg):
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    names = ("RT_TEMPORAL_SURFACE_ALPHA_MIN", "RT_TEMPORAL_SURFACE_ALPHA_SPECULAR")
    header = tuple(float(re.search(r"#define\s+" + n + r"\s+([0-9.eE+-]+)f\b", text).group(1)) for n in names)
    assert header == tuple(pkg.hip.HipScene.TEMPORAL_SURFACE_PARAMS), (header, pkg.hip.HipScene.TEMPORAL_SURFACE_PARAMS)
    for m in ("render_surface", "reproject_surface", "temporal_surface"):
        assert callable(getattr(pkg.hip.HipScene, m))


def test_surface_calls_refuse_null_arguments(pkg, abi):
    L = pkg.hip.lib()
    p = C.c_void_p(64)   # (never dereferenced: every call below is refused before it looks at a buffer)
    cam = (C.c_double * 12)()
    assert L.rt_hip_render_surface(None, None, p, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_reproject_surface(None, p, p, p, p, p, p, cam, None, 0.1, 1.0, 32.0, 0.1, 0.1, 0.1, p, None) == abi.RT_ERR_INVALID
    assert L.rt_hip_temporal_surface(None, 1, 1.0) == abi.RT_ERR_INVALID


@pytest.mark.parametrize("h,w", TC.SIZES)
def test_cpu_step_matches_numpy(step, h, w):
    rng = np.random.default_rng(1000 * h + w)
    lin, aov, prev_hist, prev_aov = TC.crafted(rng, h, w)
    surf, prev_surf = SC.crafted_surface(rng, aov, h, w)
    disps = SC.displacements(rng)
    seen = {"history": False, "none": False, "depth_cut": False, "id_cut": False, "moved_differs": False}
    for name, (cam, prev_cam) in TC.camera_pairs().items():
        for params in SC.PARAMS:
            got = {}
            for dname, disp in disps.items():
                got[dname] = step.reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, disp, params)
                want = R.reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, disp, *params)
                _same_hist(got[dname], want, (h, w, name, params, dname))
            _same_hist(got["null"], got["zero"], (h, w, name, params, "a NULL table and a table of zeros"))
            seen["moved_differs"] |= bool((_bits(got["moved"]) != _bits(got["null"])).any())
            g = got["null"]
            nan_px = np.isnan(lin).any(-1)
            assert np.array_equal(_bits(g[nan_px][:, :3]), _bits(lin[nan_px])) and (g[nan_px][:, 3] == 0).all(), "a NaN pixel: out = c, n = 0"
            assert not np.isnan(g[~nan_px]).any(), (h, w, name, params, "a NaN was written")
            n = g[~nan_px][:, 3]
            assert ((n >= 1) & (n <= F(params[2]))).all()
            fresh = n == 1
            assert np.array_equal(_bits(g[~nan_px][fresh][:, :3]), _bits(lin[~nan_px][fresh]))
            if name == "behind" or h == 1 or w == 1:
                assert fresh.all(), (h, w, name, params)
            seen["none"] |= bool(fresh.any())
            if name == "identical" and params[3] > 1e29:
                seen["history"] |= bool((n > 1).any())
            specular = ((surf["kind"] == 1) | (surf["kind"] == 2))[~nan_px]
            if params[1] == 1.0:     # alpha_specular = 1: a Metal or Glass pixel holds this frame's colour, to the roundings of hist + 1 (c - hist)
                assert np.allclose(g[~nan_px][specular][:, :3], lin[~nan_px][specular], rtol=0, atol=2e-7)
            if params[0] == 1.0:
                assert np.allclose(g[~nan_px][~specular][:, :3], lin[~nan_px][~specular], rtol=0, atol=2e-7)
        if name == "identical" and h > 1 and w > 1:   # the depth limit and the id test each reject taps the others accept
            huge = step.reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, None, (0.0, 0.0, 1e30, 1e30, 1e30, 1e30))
            cut = step.reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, None, (0.0, 0.0, 1e30, 1e30, 1e30, 0.05))
            seen["depth_cut"] |= bool(((huge[..., 3] > 1) & (cut[..., 3] == 1)).any() and (cut[..., 3] > 1).any())
            free = step.reproject(lin, aov, surf, prev_hist, prev_aov, surf, cam, prev_cam, None, (0.0, 0.0, 1e30, 1e30, 1e30, 1e30))
            seen["id_cut"] |= bool(((free[..., 3] > 1) & (huge[..., 3] == 1)).any())
    small = h == 1 or w == 1
    assert seen["none"] and (small or all(seen.values())), seen


def _centres(sc):
    return np.array([[sc.c.spheres[i].center[k] for k in range(3)] for i in range(sc.c.n_spheres)])


@pytest.mark.parametrize("name", ["cover", "test"])
def test_cpu_surface_matches_brute_force(step, load_scene, name):
    """surface_pixel through the grid walk on host-built tables against the brute force over all spheres: id, kind and the 64 bits of t"""
    sc = load_scene(name, 96, 64, 8)
    got = step.surface(sc)
    want = R.scene_surface(sc)
    _same_surf(got, want, name)
    cam = np.array(list(sc.c.cam_origin) + list(sc.c.cam_lower_left) + list(sc.c.cam_horizontal) + list(sc.c.cam_vertical))
    radii, mats = [sc.c.spheres[i].radius for i in range(sc.c.n_spheres)], [sc.c.spheres[i].kind for i in range(sc.c.n_spheres)]
    _same_surf(R.surface_all_at_once(_centres(sc), radii, mats, cam, 64, 96), want, (name, "the two forms of the brute force"))
    kinds = set(np.unique(got["kind"]).tolist())
    print(name, "kinds seen:", sorted(kinds), "sky fraction:", float((got["id"] == R.NONE).mean()))
    assert (got["id"] != R.NONE).mean() > 0.3 and len(kinds - {R.NONE}) >= 2


def test_cpu_surface_of_moving_spheres_and_thin_frames(step, load_scene):
    """every sphere at shutter time 0.5 (c + (c1 - c) * 0.5), and a 1-wide and a 1-tall frame (u or v divides by zero: no hit anywhere)"""
    sc = load_scene("scenes/cover_motion_1200x800_spp128.json", 96, 64, 8)
    c1 = np.array(sc.center1(), np.float64).reshape(-1, 3)
    got = step.surface(sc, c1)
    _same_surf(got, R.scene_surface(sc, center1=c1), "cover_motion")
    still = R.scene_surface(sc)
    assert (got.view(np.uint64) != still.view(np.uint64)).any(), "the moving spheres must show"
    for w, h in ((1, 9), (9, 1)):
        thin = load_scene("cover", w, h, 4)
        _same_surf(step.surface(thin), R.scene_surface(thin), (w, h))


def test_motion_vector_against_analytic_geometry(step):
    """One camera, a ground sphere and a unit sphere displaced by a known vector between two frames.  The previous frame's history holds
    each pixel's position in its sphere's own frame (hit point - centre); fetched through the displacement it must give the current pixel's
    own object-frame position — closer than with the displacement dropped, and closer than with its sign flipped.  Ratios are printed; only
    the ordering is asserted."""
    h, w = 64, 96
    cam = TC.camera((8.0, 3.0, 3.0), (0.0, 0.5, 0.0), vfov=30.0)
    radii, kinds = np.array([1000.0, 1.0]), np.array([0, 0])
    prev_c = np.array([[0.0, -1000.0, 0.0], [0.0, 1.0, 0.0]])
    move = np.array([0.35, 0.1, -0.3])
    now_c = prev_c.copy()
    now_c[1] += move
    disp = now_c - prev_c

    def frame(centres):
        s = R.surface(centres, radii, kinds, cam, h, w)
        d = R.centre_rays(cam, h, w)
        pos = cam[0:3] + d * s["t"][..., None]
        obj = pos - centres[np.where(s["id"] == R.NONE, 0, s["id"])]
        return s, obj
    prev_s, prev_obj = frame(prev_c)
    cur_s, cur_obj = frame(now_c)
    hist = np.zeros((h, w, 4), F)
    hist[..., 0:3] = prev_obj
    hist[..., 3] = 1.0
    lin, aov = np.zeros((h, w, 3), F), np.zeros((h, w, 8), F)   # c = 0, n' = 1, alpha 0: out = hist / 2 where history was found
    on = cur_s["id"] == 1
    params = (0.0, 0.0, 1e30, 1e30, 1e30, 1e30)

    def median_error(d):
        out = step.reproject(lin, aov, cur_s, hist, aov, prev_s, cam, cam, d, params)
        ok = on & (out[..., 3] == 2.0)
        assert ok.sum() > 50, int(ok.sum())
        return float(np.median(np.linalg.norm(2.0 * out[..., 0:3].astype(np.float64) - cur_obj, axis=-1)[ok]))
    with_d, dropped, flipped = median_error(disp), median_error(None), median_error(-disp)
    print(f"median fetch error on the moved sphere: with the displacement {with_d:.3e}, dropped {dropped:.3e} (x {dropped / with_d:.1f}), "
          f"sign flipped {flipped:.3e} (x {flipped / with_d:.1f})")
    assert with_d < dropped and with_d < flipped, (with_d, dropped, flipped)


ANIM = ["--frames", "3", "--orbit", "3", "--denoise"]


@pytest.mark.parametrize("args, usage", [
    (ANIM + ["--temporal-surface"], False),
    (["--temporal-surface"] + ANIM, False),
    (ANIM + ["--temporal-alpha", "0.2"], False),                                          # alpha_min of the mode without surface tracking
    (ANIM + ["--temporal-surface", "--temporal-alpha", "0"], False),
    (ANIM + ["--temporal-surface", "--temporal-alpha-specular", "1"], False),
    (ANIM + ["--temporal-surface", "--temporal-alpha", "0.25", "--temporal-alpha-specular", "0.5"], False),
    (["--frames", "3", "--orbit", "3", "--shutter", "0.5", "--denoise", "--temporal-surface"], False),
    (ANIM + ["--temporal-alpha-specular", "0.5"], True),                                  # needs --temporal-surface
    (ANIM + ["--temporal-surface", "--temporal-alpha", "1.5"], True),                     # outside [0, 1]
    (ANIM + ["--temporal-surface", "--temporal-alpha", "-0.1"], True),
    (ANIM + ["--temporal-surface", "--temporal-alpha-specular", "2"], True),
    (ANIM + ["--temporal-surface", "--temporal-alpha", "x"], True),
    (ANIM + ["--temporal-surface", "--temporal-alpha", "nan"], True),
    (ANIM + ["--temporal-surface", "--temporal-alpha"], True),                            # no value
    (["--denoise", "--temporal-surface"], True),                                          # only in the denoised animation
    (["--denoise", "--temporal-alpha", "0.2"], True),
    (["--frames", "3", "--orbit", "3", "--temporal-surface"], True),
    (["--frames", "3", "--temporal-alpha", "0.2"], True),
    (["--passes", "4", "--denoise", "--temporal-surface"], True),
    (["--adaptive", "0.1", "--temporal-surface"], True),
    (["--temporal-surface"], True),
])
def test_cli_argument_table(pkg, tmp_path, args, usage):
    """a refused command line prints the usage line and returns 0 before anything is read; an accepted one goes on to read the scene
    file — which does not exist here"""
    r = subprocess.run([EXE, str(tmp_path / "missing.json"), str(tmp_path / "out")] + args, capture_output=True, text=True, timeout=60)
    if usage:
        assert r.returncode == 0 and r.stdout.startswith("Usage:"), (args, r.returncode, r.stdout, r.stderr)
    else:
        assert r.returncode == 101 and "Unable to read config file" in r.stderr and "Usage" not in r.stdout, (args, r.returncode, r.stdout, r.stderr)


def test_diffuse_scene_is_what_its_generator_writes(load_scene, abi):
    """scenes/cover_diffuse_1200x800_spp128.json (the measurements' scene without mirrors and glass): the committed file is the generator's
    output, the cover's spheres where they were, every one Lambertian"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_diffuse_scene", os.path.join(ROOT, "scenes", "make_diffuse_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert open(mod.OUT).read() == mod.make()
    sc, cover = load_scene(mod.OUT), load_scene("cover")
    assert sc.c.n_spheres == cover.c.n_spheres and (_centres(sc) == _centres(cover)).all()
    assert all(sc.c.spheres[i].kind == abi.RT_MAT_LAMBERTIAN for i in range(sc.c.n_spheres))
    assert any(cover.c.spheres[i].kind == abi.RT_MAT_GLASS for i in range(cover.c.n_spheres))
