"""rt_hip_scene_update_spheres / rt_hip_group_update_spheres: a resident scene whose spheres were moved — its grid
rebuilt on the device — against the yardstick throughout: a FRESH rt_hip_scene_create_moving at the same centres, the host builder.
Tables byte for byte, frames and counters bit for bit, walks ray for ray; a refused update leaves the scene alone."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

from adversarial_rays import ray_table
from update_worlds import WORLDS, centres_of, make_world, set_centres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scenes"))
W, H = 64, 48
QUERIES = ("grid_cells", "grid_items", "grid_wide", "grid_large", "table_bytes", "motion", "n_spheres")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tables(gs):
    from rust_raytracer_amd.hip import TABLES
    return {name: gs.table(name) for name in TABLES}, {q: gs.query(q) for q in QUERIES}


def _fresh(pkg, host, wd, step, library=None):
    """the yardstick: a new scene created from the world's RtScene with the step's centres"""
    c, c1 = wd.steps[step]
    sc = host.Scene.loads(wd.text)
    set_centres(pkg.abi, sc, c)
    return pkg.hip.HipScene(sc.ptr, 0, library=library, center1=c1), sc


def _assert_same_tables(got, want, what):
    (gt, gq), (wt, wq) = got, want
    assert gq == wq, (what, gq, wq)
    for name in wt:
        assert len(gt[name]) == len(wt[name]), (what, name, len(gt[name]), len(wt[name]))
        if gt[name] != wt[name]:
            a, b = np.frombuffer(gt[name], np.uint8), np.frombuffer(wt[name], np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: table {name} differs in {bad.size} of {a.size} bytes, first at {bad[:4].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("world", list(WORLDS))
def test_updated_tables_equal_a_fresh_scene_byte_for_byte(pkg, host, torch_cuda, monkeypatch, world):
    wd = make_world(world)
    for k, v in wd.env.items():
        monkeypatch.setenv(k, v)
    library = pkg.hip.probe_lib() if wd.env else None
    sc = host.Scene.loads(wd.text)
    gs = pkg.hip.HipScene(sc.ptr, 0, library=library)
    try:
        for step in range(len(wd.steps)):
            c, c1 = wd.steps[step]
            gs.update_spheres(c, c1)
            ref, keep = _fresh(pkg, host, wd, step, library)
            try:
                want = _tables(ref)
            finally:
                ref.close()
            _assert_same_tables(_tables(gs), want, f"{world} step {step}")
            for key, value in wd.expect[step].items():   # (the case is the one its name says)
                assert want[1][key] == value if not callable(value) else value(want[1][key]), (world, step, key, want[1][key])
    finally:
        gs.close()


def _render(gs, variant=0):
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    gs.set_option("variant", variant)
    gs.render(rgb.data_ptr(), lin.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    st = gs.wait()
    gs.set_option("variant", 0)
    return rgb.cpu().numpy(), lin.cpu().numpy().view(np.uint32), {k: st[k] for k in ("segments", "exact_tests", "grid_steps")}


def _same_frame(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _accumulated(gs, n):
    acc = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda:0")
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    gs.accumulate(acc.data_ptr(), 0, 1, None, s)
    gs.accumulate(acc.data_ptr(), 1, n - 1, None, s)
    gs.resolve(acc.data_ptr(), n, rgb.data_ptr(), lin.data_ptr(), None, s)
    gs.wait()
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), lin.cpu().numpy().view(np.uint32)


def _aovs(gs, n):
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(n, aov.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return aov.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("world", ["lattice488", "moving"])
def test_frames_and_counters_after_an_update_equal_a_fresh_scene(pkg, host, torch_cuda, world):
    wd = make_world(world)
    sc = host.Scene.loads(wd.text)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    ref = None
    try:
        _render(gs)                                   # (a frame before the update: an order learned, a launch configuration cached)
        c, c1 = wd.steps[0]
        gs.update_spheres(c, c1)
        ref, keep = _fresh(pkg, host, wd, 0)
        for variant in (0, 1):
            got, want = _render(gs, variant), _render(ref, variant)
            assert _same_frame(got, want), (world, variant, got[2], want[2])
            assert want[2]["segments"] > W * H
        assert (want[2]["grid_steps"] == 0) and _render(ref, 0)[2]["grid_steps"] > 0      # (variant 1 walks no grid, variant 0 does)
        n = keep.c.samples_per_pixel
        a, b = _accumulated(gs, n), _accumulated(ref, n)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), world
        assert np.array_equal(a[0], _render(ref)[0]), world
        assert np.array_equal(_aovs(gs, n), _aovs(ref, n)), world
    finally:
        gs.close()
        if ref is not None:
            ref.close()


@pytest.mark.gpu
def test_group_update_equals_a_fresh_scene(pkg, host, torch_cuda, monkeypatch):
    """three emulated ranks, each with a second view: both follow the update (frames through the scenes and through the views)"""
    wd = make_world("moving")
    sc = host.Scene.loads(wd.text)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(sc.ptr, 3)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    ref = None
    try:
        assert grp.size == 3
        grp.render_to_host()
        c, c1 = wd.steps[0]
        out = np.zeros((H, W, 3), np.uint8)
        grp.submit(out)
        with pytest.raises(pkg.host.RtError) as e:    # a submitted frame is uncollected
            grp.update_spheres(c, c1)
        assert e.value.code == pkg.abi.RT_ERR_INVALID
        grp.collect()
        grp.update_spheres(c, c1)
        ref, keep = _fresh(pkg, host, wd, 0)
        want = _render(ref)
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])  # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want[0])
            assert {k: st[k] for k in want[2]} == want[2]
    finally:
        grp.close()
        if ref is not None:
            ref.close()


@pytest.mark.gpu
def test_round_trip_returns_to_the_first_tables(pkg, host, torch_cuda):
    wd = make_world("lattice488")
    rng = np.random.default_rng(5)
    A = wd.base
    B = A + rng.uniform(-0.3, 0.3, A.shape)
    Cc = A * 1.7 + np.array([3.0, 0.0, -2.0])
    sc = host.Scene.loads(wd.text)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    try:
        first = _tables(gs)
        for c, c1 in ((A, None), (B, B + 0.05), (Cc, None), (A, None)):
            gs.refine_to_host(1)
            assert gs.query("accum_samples") == 1
            gs.update_spheres(c, c1)
            assert gs.query("accum_samples") == 0
        _assert_same_tables(_tables(gs), first, "A -> B -> C -> A")
    finally:
        gs.close()


@pytest.mark.gpu
def test_walks_through_updated_tables_equal_a_fresh_scene(pkg, host, torch_cuda):
    wd = make_world("lattice488")
    sc = host.Scene.loads(wd.text)
    probe = pkg.hip.probe_lib()
    gs = pkg.hip.HipScene(sc.ptr, 0, library=probe)
    c, c1 = wd.steps[0]
    gs.update_spheres(c, c1)
    ref, keep = _fresh(pkg, host, wd, 0, probe)
    try:
        n = 4096
        from adversarial_rays import FAMILIES
        rays, _ = ray_table(np.random.default_rng(8), keep.c.spheres, keep.c.n_spheres, n, tuple(range(FAMILIES)))
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
        res = []
        for s in (gs, ref):
            t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
            b = torch.full((n,), -2, dtype=torch.int32, device="cuda:0")
            s.walk_probe(d_rays.data_ptr(), t.data_ptr(), b.data_ptr(), n, 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res.append((t.cpu().numpy().view(np.int64), b.cpu().numpy()))
        assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][0], res[1][0])
        assert (res[1][1] >= 0).sum() > n // 10
    finally:
        gs.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nan_motion", "moving_light", "medium_wide", "has_view"])
def test_a_refused_update_leaves_the_scene_alone(pkg, host, abi, torch_cuda, monkeypatch, case):
    wd = make_world("medium_crowd" if case == "medium_wide" else "lit30")
    sc = host.Scene.loads(wd.text)
    c = wd.base.copy()
    c1 = None
    code = abi.RT_ERR_INVALID
    if case == "nan_motion":
        c1 = c.copy(); c1[4, 1] = np.inf
    elif case == "moving_light":
        c1 = c.copy(); c1[wd.light, 0] += 0.5
    elif case == "medium_wide":
        c = wd.steps[1][0]; code = abi.RT_ERR_UNSUPPORTED
    view, L = None, pkg.hip.lib()
    gs = pkg.hip.HipScene(sc.ptr, 0)
    try:
        if case == "has_view":   # a second view of the scene's tables, made the way a group makes its ranks' views (an internal C++ entry point)
            nm = subprocess.run(["nm", "-D", "--defined-only", pkg.hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
            sym = [l.split()[-1] for l in nm.splitlines() if "rt_hip_scene_clone_view" in l]
            assert len(sym) == 1, sym
            clone = getattr(L, sym[0])
            clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            view = C.c_void_p()
            assert clone(gs._h, C.byref(view)) == abi.RT_OK
        tables, frame = _tables(gs), _render(gs)
        with pytest.raises(pkg.host.RtError) as e:
            gs.update_spheres(c, c1)
        assert e.value.code == code, (case, e.value)
        _assert_same_tables(_tables(gs), tables, case)
        assert _same_frame(_render(gs), frame), case
        if view is not None:     # ... and once the view is gone the same call goes through
            L.rt_hip_scene_destroy(view)
            view = None
            gs.update_spheres(c, c1)
    finally:
        if view is not None:
            L.rt_hip_scene_destroy(view)
        gs.close()


MOTION_SCENE = os.path.join(ROOT, "scenes", "cover_motion_1200x800_spp128.json")


@pytest.mark.gpu
def test_cli_shutter_frames_equal_one_shot_renders_of_the_frames_scenes(pkg, torch_cuda, tmp_path):
    """`--frames 3 --shutter S`: frame f is, byte for byte, the one-shot CLI render of a scene file whose spheres go from center_f to
    center1_f (the formula of csrc/host/anim_path.h, restated here); without --shutter the three frames are the scene file's own"""
    from PIL import Image
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    env0 = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    cfg = json.load(open(MOTION_SCENE))
    cfg.update(width=W, height=H, samples_per_pixel=3, max_depth=8)
    assert sum("center1" in o for o in cfg["objects"]) > 10
    base = tmp_path / "motion.json"
    base.write_text(json.dumps(cfg))
    N = 3

    def run(*args, env=env0):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (args, r.stdout, r.stderr)

    def img(name):
        return np.asarray(Image.open(tmp_path / name).convert("RGB"))

    def frame_scene(f, S):
        out = json.loads(json.dumps(cfg))
        for o in out["objects"]:
            if "center1" not in o:
                continue
            for k in "xyz":
                c, c1 = np.float64(o["center"][k]), np.float64(o["center1"][k])
                dv = c1 - c
                o["center"][k] = float(c + dv * (np.float64(f) / np.float64(N)))
                o["center1"][k] = float(c + dv * ((np.float64(f) + np.float64(S)) / np.float64(N)))
        p = tmp_path / f"frame_{f}_{S}.json"
        p.write_text(json.dumps(out))
        return p

    run(base, tmp_path / "plain.png")
    run(base, tmp_path / "plain", "--frames", N, "--orbit", 0)
    for f in range(N):
        assert np.array_equal(img(f"plain_{f:03d}.png"), img("plain.png")), f
    for S in (0.5, 0):
        tag = f"s{S}"
        run(base, tmp_path / tag, "--frames", N, "--orbit", 0, "--shutter", S)
        for f in range(N):
            run(frame_scene(f, S), tmp_path / f"{tag}_want_{f}.png")
            assert np.array_equal(img(f"{tag}_{f:03d}.png"), img(f"{tag}_want_{f}.png")), (S, f)
        assert not np.array_equal(img(f"{tag}_000.png"), img(f"{tag}_002.png")), S     # (the spheres do go somewhere)
    # the same frames with the frames distributed over (emulated) devices, and sharded over two
    run(base, tmp_path / "dist", "--frames", N, "--orbit", 0, "--shutter", 0.5, env=dict(env0, RT_ANIM="frames", RT_GPUS="2", RT_GPUS_EMULATE="1"))
    run(base, tmp_path / "shard", "--frames", N, "--orbit", 0, "--shutter", 0.5, env=dict(env0, RT_GPUS="2", RT_GPUS_EMULATE="1", RT_GATHER="peer"))
    for f in range(N):
        assert np.array_equal(img(f"dist_{f:03d}.png"), img(f"s0.5_{f:03d}.png")), f
        assert np.array_equal(img(f"shard_{f:03d}.png"), img(f"s0.5_{f:03d}.png")), f
