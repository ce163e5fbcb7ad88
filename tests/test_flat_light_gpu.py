"""Flat primitives that emit and are sampled on the GPU, through the C ABI: 48 x 32 frames at spp 4 against the restatement
(tests/flat_light_mini.py), against the full scan and against the structure bit for bit; every lights ∧ QUADS megakernel on a scene whose
only light is a panel; the state — set, remove, set twice, updates, device memory, passes, shards, adaptive frames, the group, every
refusal; two checks that need no restatement (umbra and penumbra, colour); the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import flat_light_frames as LF
import flat_light_mini as LM
from parity import assert_parity, pooled_atol
from test_medium_gpu import _cfg, _lam, _load, _obj, _one_shot, _same, _stream
from test_quad_gpu import _quad, _room_objs

LDS, SIMPLE, HL, WIDE, ACCUM, LENS, MOTION, MEDIUM, SOLID, QUADS = (1 << b for b in range(10))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
W, H, SPP = LF.W, LF.H, LF.SPP
TABLES = ("quads", "quad_lim", "flat_bvh", "flat_bvh_order", "flat_normals", "flat_motion", "motion", "flat_lights", "lights", "mat", "matc", "geom")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _scene(pkg, sc, c1=None, lens=None, quads=None, normals=None, emit=None, bvh=False):
    gs = pkg.hip.HipScene(sc.ptr, 0, center1=c1, quads=quads, flat_bvh=bvh)
    if lens:
        gs.set_lens(*lens)
    if normals is not None:
        gs.set_flat_normals(normals)
    if emit is not None:
        gs.set_flat_lights(emit)
    return gs


def _aovs(gs, n=SPP):
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(n, aov.data_ptr(), None, _stream(torch))
    torch.cuda.synchronize()
    return aov.cpu().numpy()


def _tables(gs):
    return {name: gs.table(name) for name in TABLES}


def _frames_equal(a, b, what):
    _same(a, b, what)
    assert a[2]["segments"] == b[2]["segments"] > 0, (what, a[2]["segments"], b[2]["segments"])


def _differs(a, b):
    return not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _quv(quads):
    return np.array([list(q.q) + list(q.u) + list(q.v) for q in quads])


def _with_geometry(quads, quv):
    out = (type(quads[0]) * len(quads))(*quads)
    for k in range(len(out)):
        out[k].q[:], out[k].u[:], out[k].v[:] = quv[k, 0:3], quv[k, 3:6], quv[k, 6:9]
    return out


# ------------------------------------------------------------------ frames against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("case", LF.PARITY_CASES)
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against FlatLightMini; the scene runs a lights ∧ QUADS
    kernel; "variant" 1 and the structure of §22 give the same frame bit for bit; the first-hit records are the restatement's in every bit"""
    sc, c1, lens, quads, normals, emit = LF.world(host, case)
    gs = _scene(pkg, sc, c1, lens, quads, normals, None)
    dark = _one_shot(torch, gs)
    n_sphere_lights = gs.query("n_lights")
    assert gs.query("flat_lights") == 0 and gs.table("flat_lights") == b""
    gs.set_flat_lights(emit)
    emitters = [k for k in range(len(quads)) if (emit[k] != 0).any()]
    assert gs.query("flat_lights") == len(emitters) > 0 and gs.query("n_lights") == n_sphere_lights + len(emitters)
    assert gs.table("flat_lights") == np.array(emitters, np.uint32).tobytes()
    rgb, lin, st = _one_shot(torch, gs)
    key = gs.query("last_kernel")
    assert key & HL and key & QUADS and not key & (LDS | SIMPLE | WIDE)
    assert _differs((rgb, lin), dark), "the emission changed nothing"
    m = LF.mini_frame(oracle, abi, host, case)
    assert m["n_lights"] == gs.query("n_lights")
    print(f"{case}: max |linear diff| {float(np.abs(lin - m['lin']).max()):.3g}, segments gpu {st['segments']} mini {m['segments']} - {m['discarded']}, mean {float(lin.mean()):.4f}")
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(SPP))
    assert st["segments"] == m["segments"] - m["discarded"]
    gs.set_option("variant", 1)
    _frames_equal((rgb, lin, st), _one_shot(torch, gs), "variant 1")
    assert gs.query("last_kernel") == key
    gs.set_option("variant", 0)
    tree = _scene(pkg, sc, c1, lens, quads, normals, emit, True)
    _frames_equal((rgb, lin, st), _one_shot(torch, tree), "the structure")
    assert tree.query("flat_bvh") > 0 and tree.query("last_kernel") == key
    tree.close()
    if case in ("room_panel", "tri_lamp", "box_lamp"):
        want = LF.mini(oracle, abi, sc, c1, lens, quads, normals, emit).aovs(SPP)
        got = _aovs(gs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
        k = emitters[0]
        assert (np.abs(want[..., :3] - emit[k]).max(axis=2) == 0).any(), "no pixel of the frame sees only the lamp"
    gs.close()


# ------------------------------------------------------------------ every lights ∧ QUADS megakernel
@pytest.mark.gpu
def test_all_lit_quads_kernels_with_a_panel_as_the_only_light(pkg, abi, oracle, host, torch_cuda):
    """the 16 unlit cells of test_quad_gpu's sweep, the top face of their box made a lamp: each reports its key with HL, its accumulating
    twin that key with ACCUM — the 32 lights ∧ QUADS instantiations — each frame is the restatement's at the parity bar with the exact
    segment count, the passes are the one-shot frame and the grid walk is the full scan, bit for bit"""
    import test_quad_gpu as QG
    seen = set()
    L = oracle.lib(abi)
    for cell in QG.SWEEP_CELLS:
        if cell[0]:
            continue
        name = QG.sweep_name(cell)
        sc, c1, lens, quads = QG.sweep_world(host, cell, 36, 24)
        emit = np.zeros((len(quads), 3), np.float32)
        emit[5] = (1.0, 0.8, 0.6)                      # the box's top face (the floor, then front, right, back, left, top, bottom)
        gs = _scene(pkg, sc, c1, lens, quads, None, emit)
        want = QG.sweep_key(cell) | HL
        one = _one_shot(torch, gs)
        assert gs.query("last_kernel") == want and gs.query("n_lights") == 1, (name, gs.query("last_kernel"), want)
        seen.add(want)
        mini = LM.FlatLightMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), c1, lens, quads, None, None, emit)
        m_rgb, m_lin, m_segs = mini.render()
        assert_parity(one[0], one[1], m_rgb, m_lin, name, atol=pooled_atol(2))
        assert one[2]["segments"] == m_segs - mini.discarded, name
        acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
        segs = 0
        for b, e in ((1, 2), (0, 1)):
            gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
            segs += gs.wait()["segments"]
        assert gs.query("last_kernel") == want | ACCUM, (name, gs.query("last_kernel"))
        seen.add(want | ACCUM)
        rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
        gs.resolve(acc.data_ptr(), 2, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
        torch.cuda.current_stream().synchronize()
        _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), f"{name}: accumulated vs one-shot")
        assert segs == one[2]["segments"], name
        gs.set_option("variant", 1)
        _frames_equal(one, _one_shot(torch, gs), f"{name}: variant 1")
        gs.close()
    assert seen == {QUADS | HL | s | me | m | l | a for s in (0, SOLID) for me in (0, MEDIUM) for m in (0, MOTION) for l in (0, LENS) for a in (0, ACCUM)}


@pytest.mark.gpu
def test_the_sphere_lamp_room_keeps_its_kernel_and_its_frame(pkg, abi, host, torch_cuda):
    """the lit room of tests/test_quad_gpu.py: the key it reported, and after set_flat_lights with all zeros the same tables and frame"""
    sc, c1, lens = _load(host, _cfg(_room_objs(), sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0)), W, H, SPP, 8, seed=5)
    quads = sc.quads()
    gs = _scene(pkg, sc, quads=quads)
    before, tables = _one_shot(torch, gs), _tables(gs)
    assert gs.query("last_kernel") == QUADS | HL and gs.query("n_lights") == 1 and gs.query("flat_lights") == 0
    gs.set_flat_lights(np.zeros((len(quads), 3), np.float32))
    assert _tables(gs) == tables
    _frames_equal(_one_shot(torch, gs), before, "all zeros")
    assert gs.query("last_kernel") == QUADS | HL
    gs.set_flat_lights(None)
    _frames_equal(_one_shot(torch, gs), before, "None")
    gs.close()


# ------------------------------------------------------------------ state
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_set_and_remove(pkg, abi, host, torch_cuda, bvh):
    """emission set and then removed (all zeros, or None): tables byte for byte and frames bit for bit those of a scene that never had any;
    with emission only the emitters' material records and the light list differ; set twice replaces the whole table; device memory"""
    sc, c1, lens, quads, normals, emit = LF.world(host, "room_panel")
    never = _scene(pkg, sc, c1, lens, quads, normals, None, bvh)
    gs = _scene(pkg, sc, c1, lens, quads, normals, emit, bvh)
    want_t, want_f, key = _tables(never), _one_shot(torch, never), never.query("last_kernel")
    assert key == QUADS                                    # the room without its lamp is unlit
    lit = _one_shot(torch, gs)
    assert gs.query("last_kernel") == QUADS | HL and _differs(lit, want_f)
    got_t = _tables(gs)
    k = int(np.nonzero((emit != 0).any(axis=1))[0][0])
    for name in TABLES:
        if name in ("mat", "matc"):
            size = len(got_t[name]) // (sc.c.n_spheres + len(quads))
            a, b = np.frombuffer(got_t[name], np.uint8).reshape(-1, size), np.frombuffer(want_t[name], np.uint8).reshape(-1, size)
            changed = np.nonzero((a != b).any(axis=1))[0]
            assert list(changed) == [sc.c.n_spheres + k], (name, changed)
            rec = np.frombuffer(a[sc.c.n_spheres + k].tobytes()[:16], np.uint32)
            assert rec[3] == abi.RT_MAT_LIGHT and rec[:3].tobytes() == emit[k].tobytes()
        elif name == "lights":
            assert np.frombuffer(got_t[name], np.uint32).tolist() == [sc.c.n_spheres + k] and want_t[name] == b""
        elif name == "flat_lights":
            assert np.frombuffer(got_t[name], np.uint32).tolist() == [k]
        else:
            assert got_t[name] == want_t[name], name
    gs.set_flat_lights(np.zeros_like(emit))
    assert gs.query("flat_lights") == 0 and gs.query("n_lights") == 0 and _tables(gs) == want_t
    _frames_equal(_one_shot(torch, gs), want_f, "removed")
    assert gs.query("last_kernel") == key
    other = np.zeros_like(emit); other[0] = (0.2, 0.4, 0.9)       # the floor glows instead: the panel is white Lambertian again
    gs.set_flat_lights(emit)
    gs.set_flat_lights(other)
    fresh = _scene(pkg, sc, c1, lens, quads, normals, other, bvh)
    assert _tables(gs) == _tables(fresh)
    _frames_equal(_one_shot(torch, gs), _one_shot(torch, fresh), "set twice")
    gs.set_flat_lights(torch.from_numpy(emit).to("cuda:0"))       # ... and back, from device memory
    assert _tables(gs) == got_t
    _frames_equal(_one_shot(torch, gs), lit, "from a tensor")
    gs.set_flat_lights(None)
    assert _tables(gs) == want_t
    gs.close(); never.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["scan", "refit", "rebuild"])
def test_update_flats_moves_the_lamp(pkg, abi, host, torch_cuda, route):
    """rt_hip_scene_update_flats moving the panel sideways: the aim reads the resident record, so tables and frame are those of a fresh scene
    created at the new place with the same emit — and not the frame before the move"""
    sc, c1, lens, quads, normals, emit = LF.world(host, "room_panel")
    bvh = route != "scan"
    k = int(np.nonzero((emit != 0).any(axis=1))[0][0])
    quv1 = _quv(quads)
    quv1[k, 0] += 0.9
    gs = _scene(pkg, sc, c1, lens, quads, normals, emit, bvh)
    before = _one_shot(torch, gs)
    gs.update_flats(quv1, rebuild=route == "rebuild")
    assert gs.query("flat_lights") == 1 and gs.query("n_lights") == 1
    fresh = _scene(pkg, sc, c1, lens, _with_geometry(quads, quv1), normals, emit, bvh)
    got, want = _one_shot(torch, gs), _one_shot(torch, fresh)
    a, b = _tables(gs), _tables(fresh)
    for name in ("quads", "quad_lim", "flat_lights", "lights", "mat", "matc"):
        assert a[name] == b[name], (route, name)
    _frames_equal(got, want, route)
    assert _differs(got, before)
    gs.close(); fresh.close()


@pytest.mark.gpu
def test_update_spheres_and_normals_keep_the_lamp(pkg, abi, host, torch_cuda):
    sc, c1, lens, quads, normals, emit = LF.world(host, "panel_sphere")
    gs = _scene(pkg, sc, c1, lens, quads, normals, emit)
    before = _one_shot(torch, gs)
    assert gs.query("n_lights") == 2 and gs.query("flat_lights") == 1
    centres = np.array([list(s.center) for s in sc.c.spheres[:sc.c.n_spheres]])
    moved = centres.copy(); moved[0, 0] += 0.7                   # the Light sphere itself moves between frames: light 0 is aimed at where it is
    gs.update_spheres(moved)
    assert gs.query("n_lights") == 2 and gs.query("flat_lights") == 1
    after = _one_shot(torch, gs)
    assert _differs(after, before)
    gs.update_spheres(centres)
    _frames_equal(_one_shot(torch, gs), before, "spheres back")
    gs.set_flat_normals(None)
    _frames_equal(_one_shot(torch, gs), before, "normals removed from a scene without any")
    gs.close()


@pytest.mark.gpu
def test_composition_is_the_one_shot_frame(pkg, abi, host, torch_cuda):
    """a second render, passes (0, 1), (1, 3), (3, 4), row shards {8, r, 3} and rt_hip_render_adaptive_to_host at threshold 0: each the
    one-shot frame"""
    sc, c1, lens, quads, normals, emit = LF.world(host, "box_lamp")
    gs = _scene(pkg, sc, c1, lens, quads, normals, emit)
    one = _one_shot(torch, gs)
    assert gs.query("n_lights") == 6
    _frames_equal(_one_shot(torch, gs), one, "a second render")
    acc = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") == QUADS | HL | ACCUM
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    frame_rgb, frame_lin, segs = np.zeros_like(one[0]), np.zeros_like(one[1]), 0
    for r in range(3):
        t = abi.RtRowTiles(8, r, 3)
        rows = abi.tiles_global_rows(H, t)
        s_rgb, s_lin, st = _one_shot(torch, gs, t, len(rows))
        frame_rgb[rows], frame_lin[rows] = s_rgb, s_lin
        segs += st["segments"]
    _same(one, (frame_rgb, frame_lin), "row shards")
    assert segs == one[2]["segments"]
    ad_rgb, ad_spp, _ = gs.render_adaptive(0.0, 2)
    assert (ad_spp == SPP).all() and np.array_equal(ad_rgb, one[0])
    gs.close()


@pytest.mark.gpu
def test_group_of_two_equals_one_rank(pkg, abi, host, torch_cuda, monkeypatch):
    sc, c1, lens, quads, normals, emit = LF.world(host, "tri_lamp")
    one = _scene(pkg, sc, c1, lens, quads, normals, emit)
    want = _one_shot(torch, one)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(sc.ptr, 2, quads=quads)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    try:
        assert grp.size == 2
        dark, _ = grp.render_to_host()
        assert not np.array_equal(dark, want[0])
        bad = emit.copy(); bad[1, 2] = 1.5
        with pytest.raises(pkg.host.RtError) as e:
            grp.set_flat_lights(bad)
        assert "quad 1:" in str(e.value) and np.array_equal(grp.render_to_host()[0], dark)
        grp.set_flat_lights(emit)
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])       # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want[0]) and st["segments"] == want[2]["segments"]
        grp.set_flat_lights(None, len(quads))
        assert np.array_equal(grp.render_to_host()[0], dark)
    finally:
        grp.close(); one.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(pkg, abi, host, torch_cuda):
    sc, c1, lens, quads, normals, emit = LF.world(host, "room_panel")
    L = pkg.hip.lib()
    n = len(quads)
    k = int(np.nonzero((emit != 0).any(axis=1))[0][0])
    for bvh in (False, True):
        gs = _scene(pkg, sc, c1, lens, quads, normals, emit, bvh)
        before, tables = _one_shot(torch, gs), _tables(gs)

        def refused(needle, arr=None, count=None, flags=0, code=abi.RT_ERR_INVALID, call=None):
            arr = np.ascontiguousarray(arr if arr is not None else emit)
            with pytest.raises(pkg.host.RtError) as e:
                if call is not None:
                    call()
                else:
                    pkg.hip._check(L.rt_hip_scene_set_flat_lights(gs._h, arr.ctypes.data, len(arr) if count is None else count, flags), L)
            assert e.value.code == code and needle in str(e.value), str(e.value)
            assert _tables(gs) == tables
            _frames_equal(_one_shot(torch, gs), before, needle)
        bad = emit.copy(); bad[7, 1] = np.nan; bad[9, 0] = 2.0
        refused("quad 7:", bad)
        bad = emit.copy(); bad[3, 2] = -1e-9; bad[2, 0] = np.inf
        refused("quad 2:", bad)
        bad = emit.copy(); bad[4, 0] = np.float32(1.0) + np.finfo(np.float32).eps
        refused("quad 4:", bad)
        refused("n_quads", emit[:-1])
        refused("unknown flag", flags=4)
        refused("unknown flag", flags=abi.RT_UPDATE_FLATS_REBUILD)
        move = np.zeros((n, 3)); move[k, 1] = -0.25; move[0, 0] = 0.5
        refused(f"quad {k}:", call=lambda: gs.set_flat_motion(move))          # an emitter cannot move ...
        refused(f"quad {k}:", call=lambda: gs.set_flat_motion(torch.from_numpy(move).to("cuda:0")))
        # a second view of the scene's tables, made the way a group makes its ranks' views (an internal C++ entry point)
        nm = subprocess.run(["nm", "-D", "--defined-only", pkg.hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
        sym = [l.split()[-1] for l in nm.splitlines() if "rt_hip_scene_clone_view" in l]
        assert len(sym) == 1, sym
        clone = getattr(L, sym[0])
        clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        view = C.c_void_p()
        assert clone(gs._h, C.byref(view)) == abi.RT_OK
        try:
            refused("rt_hip_group_set_flat_lights", np.zeros_like(emit))
        finally:
            L.rt_hip_scene_destroy(view)
        gs.set_flat_lights(emit)                                   # ... and once the view is gone the same call goes through
        assert _tables(gs) == tables
        gs.close()
        # ... from either call, whichever comes second
        gs = _scene(pkg, sc, c1, lens, quads, normals, None, bvh)
        gs.set_flat_motion(move)
        moving, tables = _one_shot(torch, gs), _tables(gs)
        with pytest.raises(pkg.host.RtError) as e:
            gs.set_flat_lights(emit)
        assert f"quad {k}:" in str(e.value) and _tables(gs) == tables
        _frames_equal(_one_shot(torch, gs), moving, "a moving entry cannot emit")
        gs.close()
    with pytest.raises(pkg.host.RtError):
        pkg.hip._check(L.rt_hip_scene_set_flat_lights(None, None, 0, 0), L)


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_more_than_32_emitters_are_unsupported(pkg, abi, host, torch_cuda, bvh):
    """RT_MAX_FLAT_LIGHTS: 32 emitters are taken, the 33rd is RT_ERR_UNSUPPORTED and leaves tables and frame as they were"""
    import smooth_worlds as SW
    cfg = LF._room_cfg(LF.room(LF.panel(), extra=[SW.ico_mesh(1, (1.0, 0.3, -0.6), 0.7, _lam(0.8, 0.8, 0.8), normals=None)]))
    sc, c1, lens, quads, normals, emit = LF.world(host, "many", cfg)
    assert len(quads) == 92 and abi.RT_MAX_FLAT_LIGHTS == 32
    gs = _scene(pkg, sc, c1, lens, quads, normals, emit, bvh)
    before, tables = _one_shot(torch, gs), _tables(gs)
    many = np.zeros_like(emit); many[12:12 + 33, 1] = 0.5                # 33 faces of the mesh
    with pytest.raises(pkg.host.RtError) as e:
        gs.set_flat_lights(many)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED and "RT_MAX_FLAT_LIGHTS" in str(e.value), str(e.value)
    assert _tables(gs) == tables and gs.query("flat_lights") == 1
    _frames_equal(_one_shot(torch, gs), before, "33 emitters")
    many[12 + 32] = 0.0                                                  # 32: the cap itself
    gs.set_flat_lights(many)
    assert gs.query("flat_lights") == 32 == gs.query("n_lights") and np.frombuffer(gs.table("flat_lights"), np.uint32).tolist() == list(range(12, 44))
    gs.close()


@pytest.mark.gpu
def test_headline_scene_keeps_its_kernel(pkg, load_scene, torch_cuda):
    sc = load_scene("cover", 48, 32, 2)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    _one_shot(torch, gs)
    assert gs.query("last_kernel") == 3 and gs.query("flat_lights") == 0 and gs.table("flat_lights") == b""
    with pytest.raises(pkg.host.RtError):
        gs.set_flat_lights(np.zeros((1, 3), np.float32))              # no flat primitive
    gs.close()


# ------------------------------------------------------------------ the device aim against the host build
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["parallelogram", "triangle", "a + b at 1", "0 and the largest value below 1", "needle and skewed", "|Q|, |u| over 1e+-150"])
def test_device_aim_against_the_host_build_bit_for_bit(pkg, abi, torch_cuda, name):
    """rt_hip_flat_light_aim_probe: rt_flat_light.h compiled for the device on the CPU test's class tables (10^5 activations each, the
    crafted words included) against the host build of the same header, every bit of T.  The launch of 100 000 threads runs in workgroups
    of 192 and, a second time, of 100: neither the total nor the second size is a multiple of 64."""
    import flat_light_sim
    from test_flat_light_cpu import aim_classes
    quv, tri, words = aim_classes()[name]
    want = flat_light_sim.load(abi).aim(quv, tri, words)
    P = pkg.hip.probe_lib()
    P.rt_hip_flat_light_aim_probe.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p]
    d_quv = torch.from_numpy(np.ascontiguousarray(quv)).to("cuda:0")
    d_tri = torch.from_numpy(np.ascontiguousarray(tri, np.int32)).to("cuda:0")
    d_words = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to("cuda:0")
    n = len(quv)
    assert n % 64 != 0
    for block in (192, 100):
        d_T = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda:0")        # (eight guard rows behind the table)
        pkg.hip._check(P.rt_hip_flat_light_aim_probe(d_quv.data_ptr(), d_tri.data_ptr(), d_words.data_ptr(), d_T.data_ptr(), n, block, _stream(torch)), P)
        torch.cuda.synchronize()
        got = d_T.cpu().numpy()
        assert (got[n:] == -7.0).all(), "the probe wrote past its table"
        bad = (got[:n].view(np.uint64) != want.view(np.uint64)).any(axis=1)
        assert not bad.any(), (name, block, int(bad.sum()), got[:n][bad][:2], want[bad][:2])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tri_lamp", "panel_sphere", "box_lamp"])
def test_device_light_probe_against_the_host_build(pkg, abi, host, torch_cuda, case):
    """rt_hip_flat_light_probe: what the flat arm of lane_aim_light runs — the light list, the entry's resident record and shape, child_node,
    the draw at slot 0xFFFFFFFF, the aim — of 10 007 activations (not a multiple of 64) against the host build: its Philox words for
    (pixel, sample, child_node(node, j), 0xFFFFFFFF) through its rt_flat_light_aim on the entry's q, u, v.  A light that is a sphere gives
    NaNs.  After update_flats the probe aims at where the entry now is."""
    import flat_light_sim
    sim = flat_light_sim.load(abi)
    sc, c1, lens, quads, normals, emit = LF.world(host, case)
    P = pkg.hip.probe_lib()
    P.rt_hip_flat_light_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    gs = pkg.hip.HipScene(sc.ptr, 0, library=P, center1=c1, quads=quads)
    gs.set_flat_lights(emit)
    lights = np.frombuffer(gs.table("lights"), np.uint32)
    n_lights, n_sph = len(lights), sc.c.n_spheres
    assert n_lights == gs.query("n_lights")
    rng = np.random.default_rng(41)
    n = 10007
    act = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint64).astype(np.uint32)
    j = rng.integers(0, n_lights + 1, n).astype(np.uint32)               # (n_lights itself: past the list)
    d_act = torch.from_numpy(act.view(np.int32)).to("cuda:0")
    d_j = torch.from_numpy(j.view(np.int32)).to("cuda:0")

    def probe():
        d_T = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda:0")
        pkg.hip._check(P.rt_hip_flat_light_probe(gs._h, None, d_act.data_ptr(), d_j.data_ptr(), d_T.data_ptr(), n, _stream(torch)), P)
        torch.cuda.synchronize()
        got = d_T.cpu().numpy()
        assert (got[n:] == -7.0).all(), "the probe wrote past its table"
        return got[:n]

    def expect(quv):
        flat = (j < n_lights) & (lights[np.minimum(j, n_lights - 1)] >= n_sph)
        k = lights[np.minimum(j, n_lights - 1)].astype(np.int64) - n_sph
        words = sim.words(np.concatenate([act, j[:, None]], axis=1), sc.c.seed)
        tri = np.array([int(q.reserved) for q in quads], np.int32)
        want = sim.aim(quv[np.where(flat, k, 0)], tri[np.where(flat, k, 0)], words)
        want[~flat] = np.nan
        return want, flat
    quv = _quv(quads)
    want, flat = expect(quv)
    assert flat.sum() > n // 4 and (~flat).sum() > 100
    got = probe()
    assert np.isnan(got[~flat]).all() and np.array_equal(got[flat].view(np.uint64), want[flat].view(np.uint64))
    moved = quv.copy()
    moved[:, 0:3] += (0.3, -0.2, 0.1)
    gs.update_flats(moved)
    want2, _ = expect(moved)
    got2 = probe()
    assert np.array_equal(got2[flat].view(np.uint64), want2[flat].view(np.uint64)) and not np.array_equal(got2[flat], got[flat])
    gs.close()


# ------------------------------------------------------------------ two checks with no restatement
@pytest.mark.gpu
def test_umbra_and_penumbra(pkg, abi, host, torch_cuda):
    """LF.shadow_cfg: a strip of white floor under a thin panel with a black occluder between them.  The pixels whose whole footprint
    lies where no point of the panel is visible are exactly 0 in linear radiance and RGB8; the inner half of the penumbra — the panel's
    centre hidden, a part of it visible — receives light, and less of it than the floor that sees the whole panel (an aim at the panel's
    centre fails this: the break was made once on the CPU build of the lane code, tests/test_flat_light_cpu.py)."""
    sc, c1, lens = _load(host, LF.shadow_cfg(), LF.SHADOW_W, LF.SHADOW_H, LF.SHADOW_SPP, 8, seed=29)
    gs = _scene(pkg, sc, quads=sc.quads(), emit=sc.flat_emit())
    rgb, lin, st = _one_shot(torch, gs)
    gs.close()
    print(LF.check_shadow(sc.c, rgb, lin))


@pytest.mark.gpu
def test_colour(pkg, abi, host, torch_cuda):
    """the room with emit = (1, 0, 0): the green and blue channels of every pixel equal those of the same room with NO emitter, lit by a
    Light sphere of radius 1e-3 hidden outside the room so that n_lights, the thresholds and every draw of the camera path agree.  The
    two scenes trace the same camera paths (the trigger draws depend on n_lights alone); their light rays differ, but a light ray only
    ever ADDS to `light`, and in green and blue it adds albedo x 0 in the first scene — the panel emits none — and albedo x 0 in the second
    — the hidden sphere is only ever reached from its own box of albedo 0 (LF.colour_cfg).  So both sides are exactly +0.0 in green and blue
    while red is lit: an emitter that returned white instead of `emit` fails it."""
    sc, c1, lens, quads, normals, emit = LF.world(host, "room_panel", LF.colour_cfg(True))
    red = _one_shot(torch, _scene(pkg, sc, c1, lens, quads, normals, emit))
    sc0, _, _ = _load(host, LF.colour_cfg(False), W, H, SPP, LF.DEPTH, seed=151)
    hidden = _scene(pkg, sc0, quads=sc0.quads())
    dark = _one_shot(torch, hidden)
    assert hidden.query("n_lights") == 1 and hidden.query("flat_lights") == 0
    assert red[1][..., 0].max() > 0.0
    assert np.array_equal(red[1][..., 1:].view(np.uint32), dark[1][..., 1:].view(np.uint32))
    assert np.array_equal(red[0][..., 1:], dark[0][..., 1:])
    hidden.close()


# ------------------------------------------------------------------ the CLI
@pytest.mark.gpu
def test_cli_renders_the_example_with_its_panel(pkg, abi, host, torch_cuda, tmp_path):
    """a 48 x 32 cut of scenes/make_cornell_panel_scene.py through `raytracer`: the API frame of the same file byte for byte, and NOT the
    frame of the file with "emit" stripped (which is black: the room has no other light)"""
    from PIL import Image
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cornell_panel_scene", os.path.join(ROOT, "scenes", "make_cornell_panel_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = json.loads(mod.make())
    assert cfg == json.load(open(os.path.join(ROOT, "scenes", "cornell_panel_600x600_spp128.json")))
    cfg.update(width=W, height=H, samples_per_pixel=SPP, max_depth=8)
    assert sum("emit" in o for o in cfg["objects"]) == 1
    dark_cfg = json.loads(json.dumps(cfg))
    for o in dark_cfg["objects"]:
        o.pop("emit", None)
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    imgs = {}
    for name, c in (("lit", cfg), ("dark", dark_cfg)):
        (tmp_path / f"{name}.json").write_text(json.dumps(c))
        r = subprocess.run([EXE, str(tmp_path / f"{name}.json"), str(tmp_path / f"{name}.png")], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.stdout, r.stderr)
        imgs[name] = np.asarray(Image.open(tmp_path / f"{name}.png").convert("RGB"))
    assert imgs["dark"].max() == 0 and imgs["lit"].max() > 0, "the CLI ignored the file's emission"
    sc = host.Scene.load(str(tmp_path / "lit.json"))
    gs = _scene(pkg, sc, quads=sc.quads(), emit=sc.flat_emit())
    api, _ = gs.render_to_host()
    gs.close()
    assert np.array_equal(api, imgs["lit"])


@pytest.mark.gpu
def test_cli_flat_frames_trade_emission_and_motion(pkg, abi, host, torch_cuda, tmp_path):
    """`--frames 3 --flat-frames PREFIX` with each frame's file supplying that frame's `emit` and `move`: the panel emits, then moves while
    a wall patch emits, then emits again while the patch moves — an entry that moved in one frame emits in the next and the other way
    round.  Every frame is the one-shot CLI render of its own file byte for byte, on one device and sharded over two emulated ones."""
    from PIL import Image
    env0 = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    patch = _quad((-1.99, 0.0, -1.0), (0, 0, 1.2), (0, 1.2, 0), _lam(0.7, 0.7, 0.7))

    def frame(panel_emit, panel_move, patch_emit, patch_move):
        objs = LF.room(LF.panel()) + [json.loads(json.dumps(patch))]
        for o, e, m in ((objs[3], panel_emit, panel_move), (objs[-1], patch_emit, patch_move)):
            o.pop("emit", None)
            if e is not None:
                o["emit"] = e
            if m is not None:
                o["move"] = m
        cfg = LF._room_cfg(objs)
        cfg.update(width=W, height=H, samples_per_pixel=SPP, max_depth=8)
        return cfg
    frames = [frame([1.0, 0.9, 0.75], None, None, None), frame(None, [0.4, 0.0, 0.0], [0.2, 0.6, 1.0], None),
              frame([1.0, 0.9, 0.75], None, None, [0.0, 0.5, 0.0])]
    (tmp_path / "base.json").write_text(json.dumps(frames[0]))
    for f, cfg in enumerate(frames):
        (tmp_path / f"fr_{f:03d}.json").write_text(json.dumps(cfg))

    def run(*args, env=env0):
        r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (args, r.stdout, r.stderr)

    def img(name):
        return np.asarray(Image.open(tmp_path / name).convert("RGB"))
    for f in range(3):
        run(tmp_path / f"fr_{f:03d}.json", tmp_path / f"want_{f}.png")
    assert not np.array_equal(img("want_0.png"), img("want_1.png")) and not np.array_equal(img("want_0.png"), img("want_2.png"))
    run(tmp_path / "base.json", tmp_path / "one", "--frames", 3, "--orbit", 0, "--flat-frames", tmp_path / "fr_")
    run(tmp_path / "base.json", tmp_path / "two", "--frames", 3, "--orbit", 0, "--flat-frames", tmp_path / "fr_", env=dict(env0, RT_GPUS="2", RT_GPUS_EMULATE="1"))
    for f in range(3):
        for tag in ("one", "two"):
            assert np.array_equal(img(f"{tag}_{f:03d}.png"), img(f"want_{f}.png")), (tag, f)
