"""The three tables a flat-primitive header names — shading normals, motion (§27), images (§29) — set and cleared in every
order on one resident scene, with and without the structure: after every step the scene is the one freshly created in that state, table for
table and frame for frame.  The frame is what proves the header in front of the records: no table exposes it.  The same with a geometry
update (§24, §26) between the steps, and through a group of two ranks and their views.  48 x 32 frames at spp 2; every comparison is equality."""
import itertools

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import flat_image_frames as IF
from test_flat_image_gpu import TABLES, _frames_equal, _quv, _scene, _tables, _with_geometry
from test_medium_gpu import _one_shot

NAMES = ("normals", "motion", "images")
PAIRS = list(itertools.permutations(NAMES, 2))
QUERY = {"normals": "flat_normals", "motion": "flat_motion", "images": "flat_images"}
# The structure's own tables follow the route an update took: a refit keeps the order table of the old geometry, and a rebuild under a
# motion table sorts swept boxes where a fresh scene was built still and given its motion by refit.  There a fresh scene at the new
# geometry has another structure over the same records (the frame says that both find the same hits); everywhere else — a scan scene,
# whose two tables are empty, and a rebuild without motion, by the host or the device — the structure is the fresh scene's too.
STRUCTURE = ("flat_bvh", "flat_bvh_order")
_WORLD = {}
_FRESH = {}


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _world(host, abi):
    """the smooth_mesh world at spp 2 and what each table is set to; geometry "moved": the box and the mesh translated"""
    if not _WORLD:
        w = IF.world(host, abi, "smooth_mesh")      # (a scene object of this module's own: world() loads a new one per call)
        w["sc"].c.samples_per_pixel = 2
        assert w["move"] is None and w["emit"] is None and w["lens"] is None
        n = len(w["quads"])
        move = np.zeros((n, 3))
        move[2] = (0.3, 0.0, 0.0)         # the back wall
        move[7] = (0.0, 0.1, 0.0)         # a face of the box
        quv = _quv(w["quads"])
        quv[5:, 0:3] += (0.15, 0.05, -0.1)
        _WORLD.update(w=w, n=n, value={"normals": w["normals"], "motion": move, "images": w["images"]},
                      quads={"created": w["quads"], "moved": _with_geometry(w["quads"], quv)}, quv=quv)
    return _WORLD


def _fresh(pkg, W, bvh, state, geometry="created"):
    """(tables, frame, counts) of a scene created at `geometry` and given exactly the tables of `state`, always in the order normals,
    images, motion: computed once, left unchanged.  The reference is therefore independence of the order and the route, through the same
    setters — not an independent model of them; that is what the parity frames of the tables' own test files hold against the restatements."""
    key = (bvh, frozenset(state), geometry)
    if key not in _FRESH:
        v = W["value"]
        w = dict(W["w"], quads=W["quads"][geometry], normals=v["normals"] if "normals" in state else None, move=v["motion"] if "motion" in state else None)
        gs = _scene(pkg, w, bvh, images=v["images"] if "images" in state else None)
        frame = _one_shot(torch, gs)
        frame[0].setflags(write=False); frame[1].setflags(write=False)
        _FRESH[key] = (_tables(gs), frame, {q: gs.query(q) for q in QUERY.values()})
        gs.close()
    return _FRESH[key]


def _put(target, W, name, on, group=False):
    value = W["value"][name] if on else None
    call = {"normals": target.set_flat_normals, "motion": target.set_flat_motion, "images": target.set_flat_images}[name]
    if group and not on:
        call(None, W["n"])
    else:
        call(value)


def _is_fresh(pkg, W, gs, bvh, state, what, geometry="created", tables=TABLES):
    want_t, want_f, want_q = _fresh(pkg, W, bvh, state, geometry)
    got_t = _tables(gs)
    for name in tables:
        assert got_t[name] == want_t[name], (what, name)
    assert {q: gs.query(q) for q in QUERY.values()} == want_q, what
    _frames_equal(_one_shot(torch, gs), want_f, what)


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
@pytest.mark.parametrize("a,b", PAIRS)
def test_set_and_clear_in_every_order(pkg, abi, host, torch_cuda, bvh, a, b):
    """set A, set B, clear A, clear B from a scene without a table: after each step the fresh scene of that state"""
    W = _world(host, abi)
    gs = _scene(pkg, dict(W["w"], normals=None), bvh, images=None)
    _is_fresh(pkg, W, gs, bvh, (), "no table")
    state = []
    for name, on in ((a, True), (b, True), (a, False), (b, False)):
        _put(gs, W, name, on)
        state = state + [name] if on else [s for s in state if s != name]
        _is_fresh(pkg, W, gs, bvh, state, f"{'set' if on else 'clear'} {name} -> {sorted(state)}")
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["scan", "scan_rebuild_flag", "refit", "rebuild", "device_build"])
@pytest.mark.parametrize("a,b", PAIRS)
def test_update_flats_between_the_steps(pkg, abi, host, torch_cuda, route, a, b):
    """set A, set B, update_flats, clear A, clear B: from the update on the fresh scene at the new geometry (a scan scene ignores the flag)"""
    W = _world(host, abi)
    bvh = not route.startswith("scan")
    gs = _scene(pkg, dict(W["w"], normals=None), bvh, images=None)
    if route == "device_build":
        gs.set_option("flat_build", 1)
    _put(gs, W, a, True)
    _put(gs, W, b, True)
    _is_fresh(pkg, W, gs, bvh, (a, b), "before the update")
    builds = gs.query("flat_device_builds") if route == "device_build" else 0
    order = gs.table("flat_bvh_order")
    gs.update_flats(W["quv"], rebuild=route in ("scan_rebuild_flag", "rebuild", "device_build"))
    if route == "device_build":
        assert gs.query("flat_device_builds") == builds + 1
    if route == "refit":
        assert gs.table("flat_bvh_order") == order != b""          # (a refit keeps the live order table)
    same_structure = not bvh or (route != "refit" and "motion" not in (a, b))
    tables = TABLES if same_structure else tuple(t for t in TABLES if t not in STRUCTURE)
    _is_fresh(pkg, W, gs, bvh, (a, b), f"{route}: updated", "moved", tables)
    _put(gs, W, a, False)
    _is_fresh(pkg, W, gs, bvh, (b,), f"{route}: clear {a}", "moved", tables)
    _put(gs, W, b, False)
    _is_fresh(pkg, W, gs, bvh, (), f"{route}: clear {b}", "moved", tables)
    if route == "refit":
        assert gs.table("flat_bvh_order") == order
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
@pytest.mark.parametrize("a,b", PAIRS)
def test_group_of_two_with_views(pkg, abi, host, torch_cuda, monkeypatch, bvh, a, b):
    """two ranks and their second views: set A, set B, clear A, then the single scene's frame of {B} — from render_to_host and from two
    frames in flight, the second of which renders through the views"""
    W = _world(host, abi)
    w = W["w"]
    want = _fresh(pkg, W, bvh, (b,))[1]
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(w["sc"].ptr, 2, center1=w["c1"], quads=w["quads"], flat_bvh=bvh)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    try:
        assert grp.size == 2
        _put(grp, W, a, True, group=True)
        _put(grp, W, b, True, group=True)
        _put(grp, W, a, False, group=True)
        rgb, st = grp.render_to_host()
        assert np.array_equal(rgb, want[0]) and st["segments"] == want[2]["segments"]
        frames = [np.zeros((IF.H, IF.W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])
        stats = [grp.collect(), grp.collect()]
        for f, s in zip(frames, stats):
            assert np.array_equal(f, want[0]) and s["segments"] == want[2]["segments"]
    finally:
        grp.close()
