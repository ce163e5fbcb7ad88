"""Quads and boxes on the GPU, through the C ABI: small frames against the restatement (tests/quad_mini.py) and against the
full scan bit for bit, every one of the 64 QUADS instantiations launched, composition with passes / row shards / repeated renders /
adaptive frames / sphere updates / a group, the first-hit AOVs and the surface record bitwise, the refusals, the CLI, and two checks that
are independent of every restatement: a black occluder whose edge falls inside one pixel column, and the winding of a quad."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import quad_mini as QM
from parity import assert_parity, pooled_atol
from test_medium_gpu import _cfg, _lam, _load, _med, _obj, _one_shot, _pt, _same, _stream

QUADS, SOLID, MEDIUM, MOTION, LENS, ACCUM, HL = 512, 256, 128, 64, 32, 16, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL_SCENE = os.path.join(ROOT, "scenes", "cornell_spheres_600x600_spp128.json")
W, H, SPP = 48, 32, 4       # one workgroup's worth: the tile queue, a partial wave and the quad loop all run


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _quad(q, u, v, mat):
    return {"q": _pt(*q), "u": _pt(*u), "v": _pt(*v), "material": mat}


def _box(mn, mx, mat):
    return {"box": {"min": [float(x) for x in mn], "max": [float(x) for x in mx]}, "material": mat}


def _metal(a, fuzz):
    return {"Metal": {"albedo": list(a), "fuzz": fuzz}}


GLASS = {"Glass": {"index_of_refraction": 1.5}}


def _chk(even, odd, scale):
    return {"Checker": {"even": list(even), "odd": list(odd), "scale": scale}}


def _noi(albedo, scale, mode=None, octaves=None, seed=None):
    body = {"albedo": list(albedo), "scale": scale}
    for k, v in (("mode", mode), ("octaves", octaves), ("seed", seed)):
        if v is not None:
            body[k] = v
    return {"Noise": body}


def _floor_objs(moving=False, swap=False, floor=None, extra=()):
    """a floor quad under four spheres (diffuse, metal, glass, diffuse) and a fuzzy metal quad behind them, interleaved in the file;
    moving: two spheres move over the shutter; swap: every quad is given as (Q, v, u)"""
    mv = (lambda c, d: tuple(a + b for a, b in zip(c, d))) if moving else (lambda c, d: None)
    qd = (lambda q, u, v, m: _quad(q, v, u, m)) if swap else _quad
    return [
        qd((-7, -0.5, -7), (14, 0, 0), (0, 0, 14), floor or _lam(0.6, 0.6, 0.5)),
        _obj((0, 0.5, 0), 1.0, _lam(0.8, 0.2, 0.2), mv((0, 0.5, 0), (0.3, 0.2, 0.0))),
        _obj((2.2, 0.3, 0.5), 0.8, _metal((0.8, 0.8, 0.9), 0.05)),
        qd((-3.5, -0.5, -2.5), (7, 0, 0.5), (0.3, 2.5, 0), _metal((0.9, 0.7, 0.4), 0.2)),
        _obj((0.6, 0.0, 2.5), 0.5, GLASS),
        _obj((-2.2, 0.3, 0.0), 0.8, _lam(0.2, 0.5, 0.8), mv((-2.2, 0.3, 0.0), (-0.2, 0.0, 0.3))),
    ] + list(extra)


def _room_objs():
    """a closed room seen through its open front: five Lambertian walls (red, green, white), one box, a sphere Light under the ceiling, a
    glass ball and a diffuse ball; black sky"""
    white, red, green = _lam(0.73, 0.73, 0.73), _lam(0.65, 0.05, 0.05), _lam(0.12, 0.45, 0.15)
    return [
        _quad((-2, -1, -2), (4, 0, 0), (0, 0, 4), white),       # floor
        _quad((-2, 3, -2), (4, 0, 0), (0, 0, 4), white),        # ceiling
        _quad((-2, -1, -2), (4, 0, 0), (0, 4, 0), white),       # back
        _obj((0, 2.4, 0), 0.4, {"Light": {}}),
        _quad((-2, -1, -2), (0, 0, 4), (0, 4, 0), red),         # left
        _quad((2, -1, -2), (0, 0, 4), (0, 4, 0), green),        # right
        _box((-1.3, -1, -1.2), (-0.3, 0.6, -0.2), white),
        _obj((0.8, -0.5, 0.6), 0.5, GLASS),
        _obj((0.2, -0.7, 1.2), 0.3, _lam(0.3, 0.3, 0.8)),
    ]


LENS_KEYS = {"aperture": 0.25, "focus_dist": 6.0}
PARITY_CASES = [("floor", 8), ("floor", 50), ("room", 8), ("lens", 8), ("moving", 8), ("lens_moving", 8), ("medium", 8), ("solid", 8), ("glass", 8),
                ("mirror", 8)]
_MINI_CACHE = {}


def parity_cfg(case):
    if case == "room":
        return _cfg(_room_objs(), sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0))
    if case == "medium":    # a ball of smoke cut by the floor, and one cut by the metal quad
        return _cfg(_floor_objs(extra=[_obj((0.8, -0.3, 1.6), 0.7, _med((0.8, 0.8, 0.8), 1.5)), _obj((-1.0, 0.6, -2.2), 0.9, _med((0.9, 0.6, 0.3), 2.0))]))
    if case == "solid":     # a Checker floor and a Noise wall
        return _cfg(_floor_objs(floor=_chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 1.5),
                                extra=[_quad((-4, -0.5, -3.5), (8, 0, 0), (0, 4, 0), _noi((0.9, 0.8, 0.6), 2.0, "marble", 4, 7))]))
    if case == "glass":     # a pane between the camera and the spheres
        return _cfg(_floor_objs(extra=[_quad((-1.5, -0.5, 3.4), (3, 0, 0.4), (0, 2.2, 0), GLASS)]))
    if case == "mirror":    # a mirror wall
        return _cfg(_floor_objs(extra=[_quad((3.2, -0.5, -3), (0, 0, 6), (0, 3, 0), _metal((0.95, 0.95, 0.95), 0.0))]))
    return _cfg(_floor_objs("moving" in case), lens=LENS_KEYS if "lens" in case else None)


def parity_world(host, case, depth):
    """(host scene, center1, lens, quads) of one parity case: 48 x 32 at spp 4"""
    sc, c1, lens = _load(host, parity_cfg(case), W, H, SPP, depth, seed=41 + depth)
    assert (c1 is not None) == ("moving" in case) and (lens is not None) == ("lens" in case)
    return sc, c1, lens, sc.quads()


def _mini(oracle, abi, sc, c1=None, lens=None, quads=None):
    L = oracle.lib(abi)
    return QM.QuadMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), c1, lens, quads)


def mini_frame(oracle, abi, host, case, depth):
    """QuadMini's frame of a parity case, computed once per session and left unchanged (the CPU and the GPU tests share it)"""
    key = (case, depth)
    if key not in _MINI_CACHE:
        sc, c1, lens, quads = parity_world(host, case, depth)
        m = _mini(oracle, abi, sc, c1, lens, quads)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _MINI_CACHE[key] = (rgb, lin, segs, m.discarded)
    return _MINI_CACHE[key]


def _hip_scene(pkg, sc, c1=None, lens=None, quads=None):
    gs = pkg.hip.HipScene(sc.ptr, 0, center1=c1, quads=quads)
    if lens:
        gs.set_lens(*lens)
    return gs


@pytest.mark.gpu
@pytest.mark.parametrize("case,depth", PARITY_CASES)
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case, depth):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against QuadMini; last_kernel carries QUADS and never
    the LDS or short-colour-map bits; the full scan ("variant" 1) gives the same frame bit for bit"""
    torch = torch_cuda
    sc, c1, lens, quads = parity_world(host, case, depth)
    gs = _hip_scene(pkg, sc, c1, lens, quads)
    assert gs.query("quads") == len(quads) > 0
    rgb, lin, st = _one_shot(torch, gs)
    k = gs.query("last_kernel")
    assert k & QUADS and not k & 3 and not k & 8, k
    assert bool(k & MOTION) == ("moving" in case) and bool(k & LENS) == ("lens" in case) and bool(k & HL) == (case == "room"), k
    assert bool(k & MEDIUM) == (case == "medium") and bool(k & SOLID) == (case == "solid"), k
    m_rgb, m_lin, m_segs, m_disc = mini_frame(oracle, abi, host, case, depth)
    print(f"{case} depth {depth}: max |linear diff| {float(np.abs(lin - m_lin).max()):.3g}, segments gpu {st['segments']} mini {m_segs} - {m_disc}")
    assert_parity(rgb, lin, m_rgb, m_lin, case, atol=pooled_atol(SPP))
    assert st["segments"] == m_segs - m_disc, (st["segments"], m_segs, m_disc)
    gs.set_option("variant", 1)
    b = _one_shot(torch, gs)
    assert gs.query("last_kernel") == k
    _same((rgb, lin), b, "variant 1")
    assert b[2]["segments"] == st["segments"]
    gs.close()


def _matrix_cfg(hl, medium, solid, moving, mesh=False):
    """a small world for one cell of the QUADS matrix: a floor quad (a Checker in the SOLID cells), a small box, five spheres.  The lit
    cells keep the sky: under a black one nine tenths of a 2-sample frame are zero, and zeros agree with any reference.  mesh: with
    test_tri_gpu.TETRA as a "mesh" at object index 3, in front of the box — Lambertian, and the box's Noise in the SOLID cells: 11 flat
    primitives, 4 of them triangles, so the scene has a limit table and, with more than four entries, a structure with
    inner nodes (§22)."""
    objs = [
        _quad((-5, -0.5, -5), (10, 0, 0), (0, 0, 10), _chk((0.9, 0.9, 0.9), (0.2, 0.2, 0.2), 1.5) if solid else _lam(0.6, 0.6, 0.6)),
        _obj((0, 0.5, 0), 1.0, _lam(0.8, 0.2, 0.2), (0.2, 0.6, 0.1) if moving else None),
        _obj((1.9, 0.2, 0.6), 0.7, _metal((0.8, 0.8, 0.9), 0.1)),
        _box((-2.6, -0.5, 0.2), (-1.6, 0.4, 1.2), _noi((0.8, 0.7, 0.5), 3.0, "turbulence", 2, 5) if solid else _lam(0.3, 0.6, 0.3)),
        _obj((0.5, -0.1, 2.2), 0.4, GLASS),
    ]
    if hl:
        objs.append(_obj((0, 3.5, 1), 0.8, {"Light": {}}))
    if medium:
        objs.append(_obj((-0.8, -0.2, 1.8), 0.6, _med((0.8, 0.7, 0.6), 2.5)))
    if mesh:
        from test_tri_gpu import TETRA, _mesh     # (that module imports this one)
        objs.insert(3, _mesh(*TETRA, _noi((0.8, 0.7, 0.5), 3.0, "turbulence", 2, 5) if solid else _lam(0.3, 0.7, 0.4)))
    return _cfg(objs)


# One scene per cell of the QUADS sweep, in the sweep's order: lights x pinhole / lens x static / moving x without / with media x
# without / with solids.
SWEEP_CELLS = [(hl, with_lens, moving, medium, solid) for hl in (False, True) for with_lens in (False, True) for moving in (False, True)
               for medium in (False, True) for solid in (False, True)]
SWEEP_KEYS = {QUADS | s | me | m | l | a | h for s in (0, SOLID) for me in (0, MEDIUM) for m in (0, MOTION) for l in (0, LENS)     # the 64 QUADS
              for a in (0, ACCUM) for h in (0, HL)}                                                                               # instantiations


def sweep_name(cell):
    hl, with_lens, moving, medium, solid = cell
    return f"hl={hl} lens={with_lens} moving={moving} medium={medium} solid={solid}"


def sweep_key(cell):
    """last_kernel of a cell's one-shot frame"""
    hl, with_lens, moving, medium, solid = cell
    return QUADS | (SOLID if solid else 0) | (MEDIUM if medium else 0) | (MOTION if moving else 0) | (LENS if with_lens else 0) | (HL if hl else 0)


def sweep_world(host, cell, width, height, pinhole=False, mesh=False):
    """(host scene, center1, lens, quads) of one cell at width x height, spp 2, depth 6: _matrix_cfg's world.  pinhole: the same world
    without the cell's lens.  mesh: the cell's mesh twin (_matrix_cfg), with the cell's seed."""
    hl, with_lens, moving, medium, solid = cell
    cfg = _matrix_cfg(hl, medium, solid, moving, mesh)
    if with_lens and not pinhole:
        cfg["camera"].update(aperture=0.5, focus_dist=6.0)
    sc, c1, lens = _load(host, cfg, width, height, 2, 6, seed=2 * SWEEP_CELLS.index(cell))
    return sc, c1, lens, sc.quads()


MESH_SWAP = (0.8, 0.0, 1.7)     # from the box's place to the tetrahedron's, along the floor


def sweep_mesh_geometries(quads):
    """(G, G') of a mesh twin's flat primitives as [11, 9] q, u, v rows.  G is the file's.  In G' the tetrahedron's four entries and the
    box's six have changed places (each group translated by -/+ MESH_SWAP; the floor stays): every leaf box of a structure built over G
    moves by more than its own size."""
    assert [int(q.reserved) for q in quads] == [0] + [1] * 4 + [0] * 6, "the floor, the mesh's four triangles, the box's six faces"
    g = np.array([list(q.q) + list(q.u) + list(q.v) for q in quads], np.float64)
    moved = g.copy()
    moved[1:5, :3] -= MESH_SWAP
    moved[5:11, :3] += MESH_SWAP
    return g, moved


def with_geometry(quads, quv):
    """a copy of the records with q, u, v from quv's rows"""
    out = type(quads)()
    C.memmove(out, quads, C.sizeof(quads))
    for rec, row in zip(out, quv):
        rec.q[:], rec.u[:], rec.v[:] = row[0:3].tolist(), row[3:6].tolist(), row[6:9].tolist()
    return out


@pytest.mark.gpu
def test_every_quads_instantiation_is_launched(pkg, abi, host, torch_cuda, load_scene):
    """lights x pinhole / lens x static / moving x with / without media x with / without solids x one-shot / accumulating: the 64 QUADS
    instantiations, each selected by the scene that should reach it and reporting its key; the accumulated frame is the one-shot's and the
    grid walk is the full scan's.  A quad-free scene reports the key it always reported.  (tests/test_feature_matrix.py compares every
    one of these cells with the restatement.)"""
    torch = torch_cuda
    seen = {}
    for cell in SWEEP_CELLS:
        name, medium, solid = sweep_name(cell), cell[3], cell[4]
        sc, c1, lens, quads = sweep_world(host, cell, 9, 6)
        gs = _hip_scene(pkg, sc, c1, lens, quads)
        assert gs.query("quads") == 7 and (gs.query("solids") == 7) == solid and (gs.query("media") == 1) == medium, name
        want = sweep_key(cell)
        one = _one_shot(torch, gs)
        assert gs.query("last_kernel") == want, (name, gs.query("last_kernel"), want)
        seen.setdefault(want, name)
        acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
        segs = 0
        for b, e in ((1, 2), (0, 1)):
            gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
            segs += gs.wait()["segments"]
        assert gs.query("last_kernel") == want | ACCUM, (name, gs.query("last_kernel"))
        seen.setdefault(want | ACCUM, name)
        rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
        gs.resolve(acc.data_ptr(), 2, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
        torch.cuda.current_stream().synchronize()
        _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), f"{name}: accumulated vs one-shot")
        assert segs == one[2]["segments"], name
        gs.set_option("variant", 1)
        full = _one_shot(torch, gs)
        assert gs.query("last_kernel") == want, name
        _same(one, full, f"{name}: grid walk vs full scan")
        assert full[2]["segments"] == one[2]["segments"], name
        gs.close()
    want = SWEEP_KEYS
    assert len(want) == 64 and set(seen) == want, sorted(set(seen) ^ want)
    # the headline-like quad-free scene: tables in LDS, the short colour map, nothing else — through either entry point
    sc = load_scene("cover", 48, 32, 2)
    for quads in (None, (abi.RtQuad * 1)()):
        gs = pkg.hip.HipScene(sc.ptr, 0) if quads is None else pkg.hip.HipScene(sc.ptr, 0, quads=quads[:0])
        _one_shot(torch, gs)
        assert gs.query("last_kernel") == 3 and gs.query("quads") == 0
        assert gs.table("quads") == b""
        gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["lens_moving", "room"])
def test_composition_is_the_one_shot_frame(pkg, abi, host, torch_cuda, case):
    """passes (0, 1), (1, 3), (3, 4) through rt_hip_accumulate / rt_hip_resolve, row shards {8, r, 3}, a second render, and
    rt_hip_render_adaptive_to_host at threshold 0: each the one-shot frame bit for bit"""
    torch = torch_cuda
    sc, c1, lens, quads = parity_world(host, case, 8)
    gs = _hip_scene(pkg, sc, c1, lens, quads)
    one = _one_shot(torch, gs)
    again = _one_shot(torch, gs)
    _same(one, again, "second render")
    assert again[2]["segments"] == one[2]["segments"]
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") & QUADS and gs.query("last_kernel") & ACCUM
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    frame_rgb, frame_lin = np.zeros_like(one[0]), np.zeros_like(one[1])
    segs = 0
    for r in range(3):
        t = abi.RtRowTiles(8, r, 3)
        rows = abi.tiles_global_rows(gs.height, t)
        s_rgb, s_lin, st = _one_shot(torch, gs, t, len(rows))
        frame_rgb[rows], frame_lin[rows] = s_rgb, s_lin
        segs += st["segments"]
    _same(one, (frame_rgb, frame_lin), "row shards")
    assert segs == one[2]["segments"]
    # threshold 0: no tile ever converges, every tile gets the scene's samples per pixel: the one-shot frame
    ad_rgb, ad_spp, _ = gs.render_adaptive(0.0, 2)
    assert (ad_spp == SPP).all() and np.array_equal(ad_rgb, one[0])
    gs.close()


def _surface(torch, gs):
    from temporal_surface_ref import SURF
    buf = torch.zeros((gs.height * gs.width * 2,), dtype=torch.int64, device="cuda:0")
    gs.render_surface(buf.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    return np.ascontiguousarray(buf.cpu().numpy()).view(SURF).reshape(gs.height, gs.width)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["floor", "solid", "moving", "medium", "lens"])
def test_first_hit_aovs_and_the_surface_record(pkg, abi, oracle, host, torch_cuda, case):
    """the feature buffers and the surface record of a scene with quads are QuadMini's bit for bit: a quad's albedo by the material rule
    (a solid: the colour evaluated in the quad's frame), the stored normal, 1 / t; ids n_spheres + k, kinds RT_MAT_*"""
    torch = torch_cuda
    sc, c1, lens, quads = parity_world(host, case, 8)
    gs = _hip_scene(pkg, sc, c1, lens, quads)
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(2, aov.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    m = _mini(oracle, abi, sc, c1, lens, quads)
    want = m.aovs(2)
    got = aov.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    rec = _surface(torch, gs)
    ids, kinds, ts = m.surface()
    assert np.array_equal(rec["id"], ids) and np.array_equal(rec["kind"], kinds) and np.array_equal(rec["t"].view(np.uint64), ts.view(np.uint64))
    n = sc.c.n_spheres
    on_quad = (ids >= n) & (ids != QM.SURFACE_NONE)
    assert on_quad.any() and (ids[on_quad] < n + len(quads)).all() and (ids < n).any()
    assert set(np.unique(kinds[on_quad]).tolist()) <= {q.kind for q in quads}
    gs.close()


@pytest.mark.gpu
def test_denoise_and_a_temporal_surface_step_run(pkg, abi, host, torch_cuda):
    """--denoise's call and two frames of --temporal-surface on a scene with quads: they run to completion with finite output"""
    torch = torch_cuda
    sc, c1, lens, quads = parity_world(host, "room", 8)
    gs = _hip_scene(pkg, sc, c1, lens, quads)
    frame, _ = gs.refine_to_host_denoised(4)
    assert frame.shape == (H, W, 3) and frame.any()
    gs.temporal_surface(True)
    for f in range(2):
        out, _ = gs.render_frame_temporal_to_host(f, 2)
    hist = gs.temporal_history()
    assert out.any() and np.isfinite(hist).all() and (hist[..., 3] >= 1.0).all()
    gs.close()


@pytest.mark.gpu
def test_update_spheres_keeps_the_quads(pkg, abi, host, torch_cuda):
    """rt_hip_scene_update_spheres then a render = a fresh scene with those centres and the same quads, bit for bit (tables included)"""
    torch = torch_cuda
    sc, _, _, quads = parity_world(host, "floor", 8)
    n = sc.c.n_spheres
    c0 = np.array([list(sc.c.spheres[i].center) for i in range(n)])
    new = c0 + np.array([[0.3, 0.1, -0.2], [-0.1, 0.2, 0.3], [0.2, 0.0, 0.1], [0.0, 0.3, -0.3]])
    new1 = new + np.array([[0.0, 0.2, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 0.2]])
    gs = _hip_scene(pkg, sc, None, None, quads)
    _one_shot(torch, gs)
    before = gs.table("quads")
    gs.update_spheres(new, new1)
    moved = _one_shot(torch, gs)
    assert gs.query("quads") == len(quads) and gs.query("last_kernel") == QUADS | MOTION and gs.table("quads") == before
    for i in range(n):
        sc.c.spheres[i].center[:] = new[i]
    fresh = _hip_scene(pkg, sc, new1.tolist(), None, quads)
    want = _one_shot(torch, fresh)
    _same(moved, want, "updated vs fresh")
    assert moved[2]["segments"] == want[2]["segments"]
    for name in ("geom", "motion", "cell_word", "cell_items", "large", "quads"):
        assert gs.table(name) == fresh.table(name), name
    assert len(before) == 128 * len(quads)
    gs.close(); fresh.close()


@pytest.mark.gpu
def test_a_group_of_two_is_one_rank(pkg, abi, host, torch_cuda):
    from test_gpu_parity import _with_env
    sc, c1, lens, quads = parity_world(host, "moving", 8)
    gs = _hip_scene(pkg, sc, c1, None, quads)
    want, st = gs.render_to_host()
    gs.close()
    for world in (1, 2):
        grp = _with_env({"RT_GPUS_EMULATE": "1"}, lambda: pkg.hip.HipGroup(sc.ptr, world, center1=c1, quads=quads))
        assert grp.size == world
        out, gst = grp.render_to_host()
        assert np.array_equal(out, want) and gst["segments"] == st["segments"], world
        grp.close()


def _one_quad(abi, kind=0, **kw):
    q = abi.RtQuad()
    q.q[:] = [-1.0, -1.0, 0.0]; q.u[:] = [2.0, 0.0, 0.0]; q.v[:] = [0.0, 2.0, 0.0]
    q.albedo[:] = [0.5, 0.5, 0.5]
    q.kind, q.h_offset, q.tex_w, q.tex_h, q.tex_id, q.fuzz_or_ior = kind, 2.0, 7, 0, 0, 1.5
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            getattr(q, k)[:] = v
        else:
            setattr(q, k, v)
    return q


@pytest.mark.gpu
def test_refusals(pkg, abi, host, torch_cuda):
    """more than RT_MAX_QUADS and quads with wide tables are unsupported; bad records and Texture / Light / Medium quads are invalid"""
    import fuzz_worlds as FW
    sc, _, _ = _load(host, _cfg([_obj((0, 0, 0), 1.0, _lam(0.5, 0.5, 0.5))]), 8, 8, 1, 2)
    ok = pkg.hip.HipScene(sc.ptr, 0, quads=[_one_quad(abi)] * abi.RT_MAX_QUADS)
    assert ok.query("quads") == abi.RT_MAX_QUADS
    ok.close()
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0, quads=[_one_quad(abi)] * (abi.RT_MAX_QUADS + 1))
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
    for kind in (abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_GLASS, abi.RT_MAT_CHECKER, abi.RT_MAT_NOISE):
        gs = pkg.hip.HipScene(sc.ptr, 0, quads=[_one_quad(abi, kind)])
        assert gs.query("quads") == 1 and gs.query("solids") == int(kind >= abi.RT_MAT_CHECKER)
        gs.close()
    bad = [dict(kind=abi.RT_MAT_TEXTURE), dict(kind=abi.RT_MAT_LIGHT), dict(kind=abi.RT_MAT_MEDIUM), dict(kind=8),
           dict(q=[float("nan"), 0, 0]), dict(u=[float("inf"), 0, 0]), dict(v=[0, float("-inf"), 0]),
           dict(v=[4.0, 0.0, 0.0]), dict(u=[0.0, 0.0, 0.0]), dict(u=[1e-160, 0, 0], v=[0, 1e-160, 0]), dict(u=[1e160, 0, 0], v=[0, 1e160, 0]),
           dict(kind=abi.RT_MAT_CHECKER, h_offset=0.0), dict(kind=abi.RT_MAT_NOISE, h_offset=float("nan")), dict(kind=abi.RT_MAT_NOISE, tex_w=0),
           dict(kind=abi.RT_MAT_NOISE, tex_w=17), dict(kind=abi.RT_MAT_NOISE, tex_id=3), dict(kind=abi.RT_MAT_NOISE, tex_h=1 << 32)]
    for kw in bad:
        with pytest.raises(pkg.host.RtError) as e:
            pkg.hip.HipScene(sc.ptr, 0, quads=[_one_quad(abi), _one_quad(abi, **kw)])
        assert e.value.code == abi.RT_ERR_INVALID and "quad 1" in str(e.value), (kw, str(e.value))
    big, _, _ = _load(host, json.loads(FW.big_flat_world_json(66000, np.random.default_rng(1), 8, 8, 1, 2, half=130.0)))
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(big.ptr, 0, quads=[_one_quad(abi)])
    assert e.value.code == abi.RT_ERR_UNSUPPORTED and "wide" in str(e.value)


@pytest.mark.gpu
def test_cli_renders_a_cut_of_the_cornell_example(pkg, host, torch_cuda, tmp_path):
    """the CLI's PNG of scenes/cornell_spheres_600x600_spp128.json at 48 x 32 decodes to the library call's bytes"""
    from PIL import Image
    torch = torch_cuda
    cfg = json.load(open(CORNELL_SCENE))
    cfg.update(width=W, height=H, samples_per_pixel=4)
    p = tmp_path / "cornell.json"
    p.write_text(json.dumps(cfg))
    sc, c1, ln = _load(host, cfg)
    gs = _hip_scene(pkg, sc, c1, ln, sc.quads())
    want = _one_shot(torch, gs)[0]
    assert gs.query("last_kernel") & QUADS and gs.query("last_kernel") & HL and gs.query("quads") == 17
    gs.close()
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    r = subprocess.run([exe, str(p), str(tmp_path / "cornell.png")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "cornell.png")), want)
    assert want.any()


# ------------------------------------------------------------------ exact checks with no restatement
OCC_W, OCC_H, OCC_C = 48, 32, 29


def occluder_scene(abi, with_quad):
    """Gradient sky, one far-away sphere behind the camera (no sphere in view), the pinhole at the origin looking down -z with a viewport
    of 3 x 2 at z = -1: pixel x + jitter maps to u = (x + jitter) / 47, the column's world abscissa at z = -1 is -1.5 + 3 u, so pixel column
    c covers [-1.5 + 3 c / 47, -1.5 + 3 (c + 1) / 47].  The quad lies in the plane z = -2 (facing the pinhole), spans rows and columns far
    beyond the frame on the left, top and bottom, and its right edge is at x_e = 2 (-1.5 + 3 (c + 0.5) / 47): it projects to the middle of
    column c = 29.  Albedo (0, 0, 0), Lambertian; max_depth 2."""
    spheres = (abi.RtSphere * 1)()
    s = spheres[0]
    s.center[:] = [0.0, 0.0, 50.0]
    s.radius = 1.0
    s.albedo[:] = [0.5, 0.5, 0.5]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=OCC_W, height=OCC_H, samples_per_pixel=8, max_depth=2, sky_mode=abi.RT_SKY_GRADIENT,
                     spheres=spheres, n_spheres=1, seed=123)
    sc.cam_origin[:] = [0.0, 0.0, 0.0]
    sc.cam_lower_left[:] = [-1.5, -1.0, -1.0]
    sc.cam_horizontal[:] = [3.0, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    x_e = 2.0 * (-1.5 + 3.0 * (OCC_C + 0.5) / (OCC_W - 1))
    q = abi.RtQuad()
    q.q[:] = [-20.0, -20.0, -2.0]; q.u[:] = [x_e + 20.0, 0.0, 0.0]; q.v[:] = [0.0, 40.0, 0.0]
    q.albedo[:] = [0.0, 0.0, 0.0]
    q.kind = abi.RT_MAT_LAMBERTIAN
    return sc, spheres, ([q] if with_quad else None)


@pytest.mark.gpu
def test_black_occluder(pkg, abi, torch_cuda):
    """Every pixel left of column c — fully inside the quad — is exactly 0 in linear radiance and RGB8 (a black Lambertian hit attenuates
    whatever follows by 0: 0 * x = 0 for the finite x of a gradient sky), every pixel right of c equals the quad-free frame bit for bit
    (its rays miss the quad, and a miss changes nothing), column c alone is left out.  tests/test_quad_cpu.py confirms the geometry with the
    restatement first: no jittered ray of a column left of c can miss and none right of c can hit."""
    torch = torch_cuda
    frames = []
    for with_quad in (False, True):
        sc, keep, quads = occluder_scene(abi, with_quad)
        gs = pkg.hip.HipScene(C.pointer(sc), 0, quads=quads)
        frames.append(_one_shot(torch, gs))
        assert bool(gs.query("last_kernel") & QUADS) == with_quad
        gs.close()
    (f_rgb, f_lin, _), (q_rgb, q_lin, _) = frames
    assert not q_lin[:, :OCC_C].any() and not q_rgb[:, :OCC_C].any()
    assert not np.signbit(q_lin[:, :OCC_C]).any()
    assert np.array_equal(q_rgb[:, OCC_C + 1:], f_rgb[:, OCC_C + 1:])
    assert np.array_equal(q_lin[:, OCC_C + 1:].view(np.uint32), f_lin[:, OCC_C + 1:].view(np.uint32))
    assert f_lin[:, :OCC_C].min() > 0.3, "the quad-free frame shows the sky there"
    col = q_lin[:, OCC_C].astype(np.float64).mean() / f_lin[:, OCC_C].astype(np.float64).mean()
    assert 0.1 < col < 0.9, "about half of column c's samples hit the quad"


@pytest.mark.gpu
def test_winding(pkg, abi, host, torch_cuda):
    """The unlit floor-and-spheres frame with every (Lambertian / Metal) quad given as (Q, v, u) is the original frame bit for bit: n, N, D,
    w and den change sign exactly, t, P and the hit normal keep their bits, alpha and beta change places, and neither material reads
    front_face."""
    torch = torch_cuda
    frames = []
    for swap in (False, True):
        sc, c1, lens = _load(host, _cfg(_floor_objs(swap=swap)), W, H, SPP, 8, seed=49)
        gs = _hip_scene(pkg, sc, c1, lens, sc.quads())
        frames.append(_one_shot(torch, gs))
        gs.close()
    _same(frames[0], frames[1], "swapped winding")
    assert frames[0][2]["segments"] == frames[1][2]["segments"]
