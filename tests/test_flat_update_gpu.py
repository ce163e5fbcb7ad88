"""rt_hip_scene_update_flats / rt_hip_group_update_flats on the device: a resident scene whose flat primitives were moved
against the yardstick throughout — a scene FRESHLY CREATED with the new geometry.  Tables byte for byte, frames, AOVs and surface records
bit for bit, no tolerance anywhere; the refit's boxes against the numpy refit of tests/flat_update_ref.py; a refused update leaves the
scene alone.  Frames are 48 x 32 at 4 samples per pixel."""
import ctypes as C
import subprocess

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import flat_bvh_sim as F
import flat_update_ref as U
from test_flat_bvh_gpu import _c_scene
from test_medium_gpu import _one_shot, _same, _stream

W, H, SPP = 48, 32, 4
FLAT_TABLES = ("quads", "quad_lim", "flat_bvh", "flat_bvh_order")
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _sim(abi):
    return F.load(abi)


def _flats(abi, quv, shapes=1, materials=False):
    """the entries as RtQuad records; materials: every seventh a Checker, every eleventh a Glass entry (the others Lambertian)"""
    out = F.flats_array(abi, quv, shapes)
    if materials:
        for k in range(len(out)):
            if k % 7 == 3:
                out[k].kind, out[k].h_offset = abi.RT_MAT_CHECKER, 0.75
            elif k % 11 == 5:
                out[k].kind, out[k].fuzz_or_ior = abi.RT_MAT_GLASS, 1.5
    return out


def _scene(pkg, abi, quv, shapes=1, bvh=True, materials=False, library=None):
    sc, keep = _c_scene(abi, W, H)
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=library, quads=_flats(abi, quv, shapes, materials), flat_bvh=bvh)
    gs._keep = (sc, keep)
    return gs


def _tables(gs):
    return {name: gs.table(name) for name in FLAT_TABLES}


def _assert_tables(got, want, what, names=FLAT_TABLES):
    for name in names:
        assert len(got[name]) == len(want[name]), (what, name, len(got[name]), len(want[name]))
        if got[name] != want[name]:
            a, b = np.frombuffer(got[name], np.uint8), np.frombuffer(want[name], np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: table {name} differs in {bad.size} of {a.size} bytes, first at {bad[:4].tolist()}")


def _frame(gs, variant=0):
    gs.set_option("variant", variant)
    out = _one_shot(torch, gs)
    gs.set_option("variant", 0)
    return out


def _assert_frame(got, want, what):
    _same(got, want, what)
    assert got[2]["segments"] == want[2]["segments"] > 0, what


def _differs(a, b):
    return not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _aov_surface(gs):
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
    surf = torch.zeros((H, W, 2), dtype=torch.float64, device="cuda:0")
    gs.render_aovs(SPP, aov.data_ptr(), None, _stream(torch))
    gs.render_surface(surf.data_ptr(), None, _stream(torch))
    torch.cuda.synchronize()
    return aov.cpu().numpy().view(np.uint32), surf.cpu().numpy().view(np.uint32).reshape(H, W, 4)


def _flat_share(surface, n_spheres=1):
    """the share of pixels whose surface record carries a flat primitive's id"""
    ids = surface[:, :, 0]
    return float(((ids >= n_spheres) & (ids != 0xFFFFFFFF)).mean())


# ------------------------------------------------------------------ 1. a scene without the structure
def _mixed_world():
    """32 triangles of a 4 x 4 heightfield and 5 parallelograms above it: 37 entries, both shapes"""
    from test_flat_bvh_cpu import heightfield
    tri = heightfield(n=4, size=8.0, seed=9)
    par = np.array([[-3.0 + 1.4 * k, 1.0 + 0.1 * k, -2.0 + 0.9 * k, 1.0, 0.2, 0.0, 0.0, 0.1, 1.1] for k in range(5)])
    return np.concatenate([tri, par]), np.array([1] * 32 + [0] * 5)


def _mixed_moved(quv):
    out = U.moved(quv, "ripple", 1)
    out[32:] = U.moved(quv[32:], "translate", 1)
    return out


@pytest.mark.gpu
def test_full_scan_scene_after_an_update_equals_a_fresh_scene(pkg, abi, torch_cuda):
    quv, shapes = _mixed_world()
    new = _mixed_moved(quv)
    gs = _scene(pkg, abi, quv, shapes, bvh=False, materials=True)
    ref = _scene(pkg, abi, new, shapes, bvh=False, materials=True)
    try:
        assert gs.query("quads") == 37 and gs.query("triangles") == 32 and gs.query("solids") > 0 and gs.query("flat_bvh") == 0
        before, lim = _frame(gs), gs.table("quad_lim")
        gs.update_flats(new)
        _assert_tables(_tables(gs), _tables(ref), "full scan")
        assert gs.table("quad_lim") == lim and gs.query("flat_refits") == 0
        got, want = _frame(gs), _frame(ref)
        _assert_frame(got, want, "full scan")
        assert _differs(got, before)
        a, b = _aov_surface(gs), _aov_surface(ref)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _flat_share(a[1]) >= 0.25
        gs.update_flats(quv, rebuild=True)          # (the flag means nothing without a structure: the records alone)
        _assert_frame(_frame(gs), before, "full scan, back")
    finally:
        gs.close(); ref.close()


# ------------------------------------------------------------------ 2. the structure, refit
@pytest.mark.gpu
@pytest.mark.parametrize("move", U.MOVES)
@pytest.mark.parametrize("name", ["1025", "2048"])
def test_refit_scene_equals_a_fresh_scene(pkg, abi, torch_cuda, name, move):
    sim = _sim(abi)
    base = U.world(name)
    gs = _scene(pkg, abi, base)
    ref = None
    try:
        first = _tables(gs)
        nodes0 = np.frombuffer(first["flat_bvh"], F.NODE)
        order0 = np.frombuffer(first["flat_bvh_order"], np.uint32)
        assert (nodes0["count"] == 0).any() and gs.query("flat_refits") == 0
        before = _frame(gs)
        for step in (1, 2, 3):
            new = U.moved(base, move, step)
            gs.update_flats(new)
            assert gs.query("flat_refits") == step
            t = _tables(gs)
            assert t["flat_bvh_order"] == first["flat_bvh_order"] and t["quad_lim"] == first["quad_lim"]
            want_nodes = U.refit_nodes(sim, _flats(abi, new), nodes0, order0)
            assert t["flat_bvh"] == want_nodes.tobytes(), (name, move, step)
            assert sim.check(np.frombuffer(t["flat_bvh"], F.NODE), order0, len(base)) == ""
            if step == 1:
                ref = _scene(pkg, abi, new)
                assert t["quads"] == ref.table("quads")
                got, want = _frame(gs), _frame(ref)
                _assert_frame(got, want, f"{name} {move}: refit vs fresh")
                _assert_frame(_frame(gs, 1), got, f"{name} {move}: variant 1")
                assert _differs(got, before)
                a, b = _aov_surface(gs), _aov_surface(ref)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert _flat_share(a[1]) >= 0.25, _flat_share(a[1])
        gs.update_flats(base)
        assert gs.query("flat_refits") == 4
        _assert_tables(_tables(gs), first, f"{name} {move}: back to the first geometry")
        _assert_frame(_frame(gs), before, f"{name} {move}: back")
    finally:
        gs.close()
        if ref is not None:
            ref.close()


# ------------------------------------------------------------------ 3., 4. the structure, rebuilt
@pytest.mark.gpu
def test_rebuild_flag_builds_creations_tables(pkg, abi, torch_cuda):
    base = U.world("1025")
    new = U.moved(base, "scramble", 1)
    gs, ref = _scene(pkg, abi, base), _scene(pkg, abi, new)
    try:
        gs.update_flats(U.moved(base, "ripple", 1))
        assert gs.query("flat_refits") == 1
        gs.update_flats(new, rebuild=True)
        assert gs.query("flat_refits") == 0 and gs.query("flat_bvh") == ref.query("flat_bvh")
        _assert_tables(_tables(gs), _tables(ref), "rebuild")
        _assert_frame(_frame(gs), _frame(ref), "rebuild")
        gs.update_flats(new)                        # a refit to the geometry of the build: the build's nodes
        assert gs.query("flat_refits") == 1
        _assert_tables(_tables(gs), _tables(ref), "refit after the rebuild")
    finally:
        gs.close(); ref.close()


@pytest.mark.gpu
def test_refused_set_change_rebuilds_in_both_directions(pkg, abi, torch_cuda):
    base = U.world("1025")
    thin = U.needle(base, 100)
    gs, ref = _scene(pkg, abi, base), _scene(pkg, abi, thin)
    try:
        first, before = _tables(gs), _frame(gs)
        gs.update_flats(U.moved(base, "translate", 1))
        gs.update_flats(base)
        assert gs.query("flat_refits") == 2
        gs.update_flats(thin)                       # entry 100 became a needle: the always-visited run gains a leaf
        assert gs.query("flat_refits") == 0
        want = _tables(ref)
        assert want["flat_bvh_order"] != first["flat_bvh_order"] and np.frombuffer(want["flat_bvh_order"], np.uint32)[0] == 100
        _assert_tables(_tables(gs), want, "into the refused set")
        _assert_frame(_frame(gs), _frame(ref), "needle")
        _assert_frame(_frame(gs, 1), _frame(ref), "needle, variant 1")
        gs.update_flats(U.needle(U.moved(base, "translate", 1), 100))   # the set stays: a refit, the leaf keeps its infinite box
        assert gs.query("flat_refits") == 1
        nodes = np.frombuffer(gs.table("flat_bvh"), F.NODE)
        assert np.isinf(nodes["lo"][0]).all() and np.isfinite(nodes["lo"][1:]).all()
        gs.update_flats(base)                       # ... and out of it again
        assert gs.query("flat_refits") == 0
        _assert_tables(_tables(gs), first, "out of the refused set")
        _assert_frame(_frame(gs), before, "restored")
    finally:
        gs.close(); ref.close()


# ------------------------------------------------------------------ 5. geometry in device memory
@pytest.mark.gpu
def test_device_tensor_gives_the_host_paths_tables(pkg, abi, torch_cuda):
    base = U.world("2048")
    new = U.moved(base, "ripple", 2)
    a, b = _scene(pkg, abi, base), _scene(pkg, abi, base)
    try:
        a.update_flats(new)
        b.update_flats(torch.from_numpy(new).to("cuda:0"))
        assert b.query("flat_refits") == 1
        _assert_tables(_tables(b), _tables(a), "device tensor, refit")
        thin = U.needle(new, 7)
        a.update_flats(thin)
        b.update_flats(torch.from_numpy(thin).to("cuda:0"))             # (a rebuild: the geometry is copied back first)
        assert b.query("flat_refits") == 0
        _assert_tables(_tables(b), _tables(a), "device tensor, rebuild")
        b.update_flats(torch.from_numpy(new).to("cuda:0").t().contiguous().t())   # not contiguous: through the host
        a.update_flats(new)
        _assert_tables(_tables(b), _tables(a), "strided tensor")
        _assert_frame(_frame(b), _frame(a), "device tensor")
        with pytest.raises(ValueError):
            b.update_flats(torch.zeros((2048, 9), dtype=torch.float32, device="cuda:0"))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 6. errors
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["null", "count", "no_flats", "flag", "non_finite", "degenerate", "lowest", "has_view"])
def test_a_refused_update_leaves_the_scene_alone(pkg, abi, torch_cuda, case):
    base = U.world("1025")
    L = pkg.hip.lib()
    new = U.moved(base, "ripple", 1)
    needle = ""
    if case == "non_finite":
        new[700, 4], new[900, 0], needle = np.nan, np.inf, "quad 700: q, u and v must be finite"
    elif case == "degenerate":
        new[[300, 800], 6:9], needle = new[[300, 800], 3:6], "quad 300: degenerate"
    elif case == "lowest":
        new[10, 3:9], new[5, 2], needle = 0.0, -np.inf, "quad 5: q, u and v must be finite"
    view = None
    gs = _scene(pkg, abi, base)
    try:
        tables, frame = _tables(gs), _frame(gs)
        if case == "no_flats":
            sc, keep = _c_scene(abi, W, H)
            plain = pkg.hip.HipScene(C.pointer(sc), 0)
            try:
                with pytest.raises(pkg.host.RtError) as e:
                    plain.update_flats(new)
                assert e.value.code == abi.RT_ERR_INVALID and "no flat primitive" in str(e.value)
            finally:
                plain.close()
            return
        if case == "has_view":   # a second view of the scene's tables, made the way a group makes its ranks' views (an internal C++ entry point)
            nm = subprocess.run(["nm", "-D", "--defined-only", pkg.hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
            sym = [l.split()[-1] for l in nm.splitlines() if "rt_hip_scene_clone_view" in l]
            assert len(sym) == 1, sym
            clone = getattr(L, sym[0])
            clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            view = C.c_void_p()
            assert clone(gs._h, C.byref(view)) == abi.RT_OK
            needle = "rt_hip_group_update_flats"
        with pytest.raises(pkg.host.RtError) as e:
            if case == "null":
                pkg.hip._check(L.rt_hip_scene_update_flats(gs._h, None, 1025, 0), L)
            elif case == "flag":
                pkg.hip._check(L.rt_hip_scene_update_flats(gs._h, new.ctypes.data, 1025, 4), L)
            elif case == "count":
                gs.update_flats(new[:1024])
            else:
                gs.update_flats(new)
        assert e.value.code == abi.RT_ERR_INVALID and needle in str(e.value), (case, e.value)
        assert gs.query("flat_refits") == 0
        _assert_tables(_tables(gs), tables, case)
        _assert_frame(_frame(gs), frame, case)
        if view is not None:     # ... and once the view is gone the same call goes through
            L.rt_hip_scene_destroy(view)
            view = None
            gs.update_flats(new)
            assert gs.query("flat_refits") == 1
    finally:
        if view is not None:
            L.rt_hip_scene_destroy(view)
        gs.close()


# ------------------------------------------------------------------ 7. what an update drops, what it keeps
@pytest.mark.gpu
def test_update_drops_the_accumulator_and_the_temporal_history(pkg, abi, torch_cuda):
    base = U.world("1025")
    new = U.moved(base, "ripple", 1)
    gs, ref = _scene(pkg, abi, base), _scene(pkg, abi, new)
    try:
        gs.refine_to_host(2)
        gs.render_frame_temporal_to_host(0)
        assert gs.query("accum_samples") == 2 and gs.temporal_history().any()
        gs.update_flats(new)
        assert gs.query("accum_samples") == 0
        with pytest.raises(pkg.host.RtError):       # as after rt_hip_temporal_reset: the scene holds no history
            gs.temporal_history()
        for n in (1, 3):
            got, want = gs.refine_to_host(n), ref.refine_to_host(n)
            assert np.array_equal(got[0], want[0]) and got[1]["segments"] == want[1]["segments"]
        assert gs.query("accum_samples") == 4
        a, b = gs.render_frame_temporal_to_host(0), ref.render_frame_temporal_to_host(0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(gs.temporal_history().view(np.uint32), ref.temporal_history().view(np.uint32))
    finally:
        gs.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flats_first", [True, False])
def test_sphere_and_flat_updates_in_either_order(pkg, abi, torch_cuda, flats_first):
    base = U.world("1025")
    new = U.moved(base, "translate", 1)
    centre = np.array([[-1.0, 1.5, 0.8]])
    gs = _scene(pkg, abi, base)
    sc, spheres = _c_scene(abi, W, H)
    spheres[0].center[:] = centre[0].tolist()
    ref = pkg.hip.HipScene(C.pointer(sc), 0, quads=_flats(abi, new), flat_bvh=True)
    try:
        before = _frame(gs)
        if flats_first:
            gs.update_flats(new); gs.update_spheres(centre)
        else:
            gs.update_spheres(centre); gs.update_flats(new)
        assert gs.table("geom") == ref.table("geom")
        _assert_tables(_tables(gs), _tables(ref), "both updates", ("quads", "quad_lim"))   # (a refit tree is not the fresh build's tree)
        assert gs.query("flat_refits") == 1
        got = _frame(gs)
        _assert_frame(got, _frame(ref), "both updates")
        assert _differs(got, before)
    finally:
        gs.close(); ref.close()


# ------------------------------------------------------------------ 8. the group
@pytest.mark.gpu
def test_group_update_equals_a_fresh_scene(pkg, abi, torch_cuda, monkeypatch):
    """two emulated ranks, each with a second view: both follow the update (frames through the scenes and through the views)"""
    base = U.world("1025")
    new = U.moved(base, "ripple", 1)
    sc, keep = _c_scene(abi, W, H)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(C.pointer(sc), 2, quads=_flats(abi, base), flat_bvh=True)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    ref = _scene(pkg, abi, new)
    try:
        assert grp.size == 2
        first, _ = grp.render_to_host()
        out = np.zeros((H, W, 3), np.uint8)
        grp.submit(out)
        with pytest.raises(pkg.host.RtError) as e:    # a submitted frame is uncollected
            grp.update_flats(new)
        assert e.value.code == abi.RT_ERR_INVALID
        grp.collect()
        bad = new.copy()
        bad[3, 0] = np.nan
        with pytest.raises(pkg.host.RtError) as e:
            grp.update_flats(bad)
        assert "quad 3" in str(e.value)
        assert np.array_equal(grp.render_to_host()[0], first)
        grp.update_flats(new)
        want = _frame(ref)
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])  # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want[0]) and st["segments"] == want[2]["segments"]
        assert not np.array_equal(frames[0], first)
    finally:
        grp.close(); ref.close()


# ------------------------------------------------------------------ 9. the CLI
@pytest.mark.gpu
def test_cli_flat_frames_equal_one_shot_renders_of_the_frame_files(pkg, torch_cuda, tmp_path):
    """`--frames 3 --flat-frames PREFIX`: frame f is, byte for byte, the one-shot CLI render of the base file with that frame's flat
    primitives — which is what the frame file is; with the structure (the generator's "flat_bvh": true, and --flat-bvh on a file without
    the key) and without it, with the frames sharded over two emulated devices and distributed over them"""
    import json
    import os
    from PIL import Image
    from test_flat_update_cpu import EXE, make_flat_anim
    env0 = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    N = 3
    base, prefix = make_flat_anim().write(str(tmp_path), n=5, frames=N, width=W, height=H, spp=3)
    files = [base] + [f"{prefix}{f:03d}.json" for f in range(N)]
    plain_dir = tmp_path / "scan"
    plain_dir.mkdir()
    for p in files:                                   # the same files without the structure: 50 triangles, the full scan
        cfg = json.load(open(p))
        del cfg["flat_bvh"]
        (plain_dir / os.path.basename(p)).write_text(json.dumps(cfg))

    def run(*args, env=env0):
        r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (args, r.stdout, r.stderr)

    def img(name):
        return np.asarray(Image.open(tmp_path / name).convert("RGB"))

    for f in range(N):
        run(files[1 + f], tmp_path / f"want_{f}.png")
    assert not np.array_equal(img("want_0.png"), img("want_2.png"))                     # (the sheet does move)
    scan_base, scan_prefix = plain_dir / "flat_anim.json", str(plain_dir / "flat_anim_")
    run(base, tmp_path / "bvh", "--frames", N, "--orbit", 0, "--flat-frames", prefix)
    run(scan_base, tmp_path / "scan_out", "--frames", N, "--orbit", 0, "--flat-frames", scan_prefix)
    run(scan_base, tmp_path / "flag", "--frames", N, "--orbit", 0, "--flat-frames", scan_prefix, "--flat-bvh")
    run(base, tmp_path / "shard", "--frames", N, "--orbit", 0, "--flat-frames", prefix, env=dict(env0, RT_GPUS="2", RT_GPUS_EMULATE="1"))
    run(base, tmp_path / "dist", "--frames", N, "--orbit", 0, "--flat-frames", prefix, env=dict(env0, RT_ANIM="frames", RT_GPUS="2", RT_GPUS_EMULATE="1"))
    for f in range(N):
        for tag in ("bvh", "scan_out", "flag", "shard", "dist"):
            assert np.array_equal(img(f"{tag}_{f:03d}.png"), img(f"want_{f}.png")), (tag, f)
