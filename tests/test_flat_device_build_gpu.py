"""The flat-primitive BVH's order table built on the device (rt_hip_set_option "flat_build" 1 + RT_UPDATE_FLATS_REBUILD)
against the yardstick of §24: a scene FRESHLY CREATED with the new geometry, whose tables the host builder made.  The record, limit, node
and order tables byte for byte (the fourth resident piece, the header in front of the records, holds device addresses: it is compared
through what it serves — frames, AOVs and surface records, bit for bit).  No tolerance anywhere.  Frames are 48 x 32 at 4 samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import flat_build_worlds as B
import flat_update_ref as U
from test_flat_bvh_gpu import _c_scene
from test_flat_update_gpu import (H, W, _aov_surface, _assert_frame, _assert_tables, _differs, _flats, _frame, _scene, _tables)

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
REBUILD = 1   # RT_UPDATE_FLATS_REBUILD


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _device_scene(pkg, abi, quv, **kw):
    gs = _scene(pkg, abi, quv, **kw)
    gs.set_option("flat_build", 1)
    return gs


# ------------------------------------------------------------------ 1. the option and the two queries
@pytest.mark.gpu
def test_option_and_queries(pkg, abi, torch_cuda):
    """(the test that fails without the feature: the first set_option is refused there)"""
    base = U.world("1025")
    gs = _scene(pkg, abi, base)
    scan = _scene(pkg, abi, base[:37], bvh=False)
    ref = _scene(pkg, abi, U.moved(base[:37], "ripple", 1), bvh=False)
    try:
        assert abi.RT_UPDATE_FLATS_REBUILD == REBUILD
        assert gs.query("flat_build") == 0 and gs.query("flat_device_builds") == 0
        gs.set_option("flat_build", 1)
        assert gs.query("flat_build") == 1
        gs.set_option("flat_build", 0)
        assert gs.query("flat_build") == 0
        for bad in (2, -1, 1 << 40):
            with pytest.raises(pkg.host.RtError) as e:
                gs.set_option("flat_build", bad)
            assert e.value.code == abi.RT_ERR_INVALID and "flat_build" in str(e.value)
        assert gs.query("flat_build") == 0
        # option 0: a rebuild is the host's, as it always was
        new = U.moved(base, "ripple", 1)
        gs.update_flats(new, rebuild=True)
        assert gs.query("flat_device_builds") == 0 and "update_flats.host_build" in pkg.hip.setup_profile()
        # a scene without the structure takes the option and nothing changes: the records alone
        scan.set_option("flat_build", 1)
        assert scan.query("flat_build") == 1 and scan.query("flat_bvh") == 0
        scan.update_flats(U.moved(base[:37], "ripple", 1), rebuild=True)
        assert scan.query("flat_device_builds") == 0 and scan.query("flat_refits") == 0
        _assert_tables(_tables(scan), _tables(ref), "scan scene")
        _assert_frame(_frame(scan), _frame(ref), "scan scene")
    finally:
        gs.close(); scan.close(); ref.close()


# ------------------------------------------------------------------ 2. tables byte for byte, frames bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("move", U.MOVES)
@pytest.mark.parametrize("name", ["1025", "2048"])
def test_device_rebuild_leaves_a_fresh_scenes_tables(pkg, abi, torch_cuda, name, move):
    base = U.world(name)
    new = U.moved(base, move, 1)
    gs, ref = _device_scene(pkg, abi, base), _scene(pkg, abi, new)
    try:
        first, before = _tables(gs), _frame(gs)
        gs.update_flats(new, rebuild=True)
        assert gs.query("flat_refits") == 0 and gs.query("flat_device_builds") == 1 and gs.query("flat_bvh") == ref.query("flat_bvh")
        assert "update_flats.host_build" not in pkg.hip.setup_profile()
        got = _tables(gs)
        _assert_tables(got, _tables(ref), f"{name} {move}")
        if move == "scramble":   # (the order table is another than the resident one: a refit could not have made these tables)
            assert got["flat_bvh_order"] != first["flat_bvh_order"]
        a, b = _frame(gs), _frame(ref)
        _assert_frame(a, b, f"{name} {move}")
        assert _differs(a, before)
        x, y = _aov_surface(gs), _aov_surface(ref)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        gs.update_flats(new)                         # a refit to the geometry of the build: the build's nodes again
        assert gs.query("flat_refits") == 1
        _assert_tables(_tables(gs), got, f"{name} {move}: refit after the device build")
    finally:
        gs.close(); ref.close()


# ------------------------------------------------------------------ 3. the small worlds of the CPU test, and one large one
@pytest.mark.gpu
@pytest.mark.parametrize("name", B.SMALL + ("big",))
def test_small_and_large_worlds(pkg, abi, torch_cuda, name):
    """the scene starts scrambled (the refused entries stay refused: a scramble translates) and is rebuilt INTO the world under test, so
    the equal centres, the ties at 0.0, the three axes and the short always-visited runs are what the device splits; then back"""
    world = B.world(name)
    start = U.moved(world, "scramble", 1)
    gs, ref = _device_scene(pkg, abi, start), _scene(pkg, abi, world)
    try:
        first = _tables(gs)
        want = _tables(ref)
        n_always = len(B.NEEDLES.get(name, ()))
        assert np.frombuffer(want["flat_bvh_order"], np.uint32)[:n_always].tolist() == B.NEEDLES.get(name, [])
        gs.update_flats(world, rebuild=True)
        assert gs.query("flat_device_builds") == 1 and gs.query("flat_refits") == 0
        _assert_tables(_tables(gs), want, name)
        gs.update_flats(start, rebuild=True)
        assert gs.query("flat_device_builds") == 2
        _assert_tables(_tables(gs), first, name + ": back")
        if name == "big":
            assert len(world) == 2 ** 16 + 3 and B.depths(len(world)) == 15
            gs.update_flats(world, rebuild=True)
            _assert_frame(_frame(gs), _frame(ref), name)
    finally:
        gs.close(); ref.close()


# ------------------------------------------------------------------ 4. refit, then rebuild
@pytest.mark.gpu
def test_refits_then_a_device_rebuild(pkg, abi, torch_cuda):
    base = U.world("1025")
    new = U.moved(base, "scramble", 2)
    gs, ref = _device_scene(pkg, abi, base), _scene(pkg, abi, new)
    try:
        for step in (1, 2, 3):
            gs.update_flats(U.moved(base, "ripple", step))
        assert gs.query("flat_refits") == 3 and gs.query("flat_device_builds") == 0
        gs.update_flats(new, rebuild=True)
        assert gs.query("flat_refits") == 0 and gs.query("flat_device_builds") == 1
        _assert_tables(_tables(gs), _tables(ref), "refits, then a rebuild")
        _assert_frame(_frame(gs), _frame(ref), "refits, then a rebuild")
    finally:
        gs.close(); ref.close()


# ------------------------------------------------------------------ 5. geometry in device memory
@pytest.mark.gpu
def test_device_tensor_rebuild_copies_nothing_back(pkg, abi, torch_cuda):
    base = U.world("2048")
    new = U.moved(base, "scramble", 1)
    a, b, ref = _device_scene(pkg, abi, base), _device_scene(pkg, abi, base), _scene(pkg, abi, new)
    try:
        a.update_flats(new, rebuild=True)
        b.update_flats(torch.from_numpy(new).to("cuda:0"), rebuild=True)
        stages = pkg.hip.setup_profile()             # (the geometry is read where it lies; the one readback is the status block's)
        assert "update_flats.host_build" not in stages and "update_flats.upload_structure" not in stages, stages
        assert b.query("flat_device_builds") == 1
        _assert_tables(_tables(b), _tables(a), "device tensor")
        _assert_tables(_tables(b), _tables(ref), "device tensor vs fresh")
        _assert_frame(_frame(b), _frame(ref), "device tensor")
        b.set_option("flat_build", 0)                # ... and with the option back at 0 the same call is the host's again
        b.update_flats(torch.from_numpy(base.copy()).to("cuda:0"), rebuild=True)
        assert "update_flats.host_build" in pkg.hip.setup_profile() and b.query("flat_device_builds") == 1
    finally:
        a.close(); b.close(); ref.close()


# ------------------------------------------------------------------ 6. a changed refused set: the host builds, whatever the option says
@pytest.mark.gpu
def test_mismatch_rebuilds_on_the_host(pkg, abi, torch_cuda):
    base = U.world("1025")
    thin = U.needle(base, 100)
    moved = U.needle(U.moved(base, "scramble", 1), 100)
    gs, ref, ref2 = _device_scene(pkg, abi, base), _scene(pkg, abi, thin), _scene(pkg, abi, moved)
    try:
        gs.update_flats(thin, rebuild=True)          # entry 100 became a needle: another run, another count of boxed entries
        assert gs.query("flat_device_builds") == 0 and gs.query("flat_refits") == 0
        assert "update_flats.host_build" in pkg.hip.setup_profile()
        _assert_tables(_tables(gs), _tables(ref), "mismatch, flag set")
        _assert_frame(_frame(gs), _frame(ref), "mismatch")
        gs.update_flats(base)                        # ... and without the flag
        assert gs.query("flat_device_builds") == 0 and gs.query("flat_refits") == 0
        gs.update_flats(thin)
        _assert_tables(_tables(gs), _tables(ref), "mismatch, no flag")
        gs.update_flats(moved, rebuild=True)         # the set stays: the device builds over the new topology
        assert gs.query("flat_device_builds") == 1
        _assert_tables(_tables(gs), _tables(ref2), "device build after a host build")
    finally:
        gs.close(); ref.close(); ref2.close()


# ------------------------------------------------------------------ 7. a refused update
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["non_finite", "degenerate"])
def test_a_refused_rebuild_leaves_the_scene_alone(pkg, abi, torch_cuda, case):
    base = U.world("1025")
    new = U.moved(base, "scramble", 1)
    if case == "non_finite":
        new[700, 4], new[900, 0], needle = np.nan, np.inf, "quad 700: q, u and v must be finite"
    else:
        new[[300, 800], 6:9], needle = new[[300, 800], 3:6], "quad 300: degenerate"
    gs = _device_scene(pkg, abi, base)
    try:
        gs.update_flats(U.moved(base, "ripple", 1))
        tables, frame = _tables(gs), _frame(gs)
        with pytest.raises(pkg.host.RtError) as e:
            gs.update_flats(new, rebuild=True)
        assert e.value.code == abi.RT_ERR_INVALID and needle in str(e.value)
        assert gs.query("flat_refits") == 1 and gs.query("flat_device_builds") == 0
        _assert_tables(_tables(gs), tables, case)
        _assert_frame(_frame(gs), frame, case)
    finally:
        gs.close()


# ------------------------------------------------------------------ 8. the group
@pytest.mark.gpu
def test_group_rebuilds_on_the_device(pkg, abi, torch_cuda, monkeypatch):
    base = U.world("1025")
    new = U.moved(base, "scramble", 1)
    sc, keep = _c_scene(abi, W, H)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(C.pointer(sc), 2, quads=_flats(abi, base), flat_bvh=True)
    fresh = pkg.hip.HipGroup(C.pointer(sc), 2, quads=_flats(abi, new), flat_bvh=True)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    try:
        assert grp.size == 2
        with pytest.raises(pkg.host.RtError):
            grp.set_option("flat_build", 2)
        grp.set_option("flat_build", 1)
        first, _ = grp.render_to_host()
        grp.update_flats(new, rebuild=True)
        assert "update_flats.host_build" not in pkg.hip.setup_profile()
        want, want_stats = fresh.render_to_host()
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])  # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want) and st["segments"] == want_stats["segments"]
        assert not np.array_equal(frames[0], first)
    finally:
        grp.close(); fresh.close()


# ------------------------------------------------------------------ 9. the CLI
@pytest.mark.gpu
def test_cli_flat_rebuild_writes_the_same_pngs(pkg, torch_cuda, tmp_path):
    """`--flat-frames PREFIX --flat-rebuild 2`: the PNG files of the run without the flag, byte for byte, on one device and sharded over
    two emulated ones; refused on a scene without the structure"""
    import json
    from test_flat_update_cpu import EXE, make_flat_anim
    env0 = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    N = 5
    base, prefix = make_flat_anim().write(str(tmp_path), n=5, frames=N, width=W, height=H, spp=3)

    def run(*args, env=env0):
        return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)

    common = ("--frames", N, "--orbit", 0, "--flat-frames", prefix)
    runs = {"plain": (), "rebuild": ("--flat-rebuild", 2), "every": ("--flat-rebuild", 1)}
    for tag, extra in runs.items():
        r = run(base, tmp_path / tag, *common, *extra)
        assert r.returncode == 0 and r.stdout.count("Rendering") == N, (tag, r.stdout, r.stderr)
    r = run(base, tmp_path / "shard", *common, "--flat-rebuild", 2, env=dict(env0, RT_GPUS="2", RT_GPUS_EMULATE="1"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    r = run(base, tmp_path / "dist", *common, "--flat-rebuild", 2, env=dict(env0, RT_ANIM="frames", RT_GPUS="2", RT_GPUS_EMULATE="1"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    png = lambda tag, f: open(tmp_path / f"{tag}_{f:03d}.png", "rb").read()
    assert png("plain", 0) != png("plain", 4)
    for f in range(N):
        for tag in ("rebuild", "every", "shard", "dist"):
            assert png(tag, f) == png("plain", f), (tag, f)
    cfg = json.load(open(base))
    del cfg["flat_bvh"]
    scan = tmp_path / "scan.json"
    scan.write_text(json.dumps(cfg))
    r = run(scan, tmp_path / "scan", *common, "--flat-rebuild", 2)
    assert r.returncode == 101 and "--flat-rebuild" in r.stderr and "Rendering" not in r.stdout, (r.stdout, r.stderr)
