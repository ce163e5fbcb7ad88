"""The 24 base instantiations of the megakernel against the CPU oracle.

rt_megakernel<HL, SIMPLE, LDS, WIDE, ACCUM, LENS, MOTION, MEDIUM, SOLID, QUADS> (rt_kernel.hip) has 352 instantiations
(kernel_key_valid), one picked per launch from the scene (lights; every albedo in [0, 1]; a lens; moving spheres; media; solid
textures; flat primitives), where plan_lds puts the tables (LDS, L2, or the wide format) and whether the launch is one-shot or
accumulating.  rt_hip_scene_query("last_kernel") reports which one ran:
QUADS 512 | SOLID 256 | MEDIUM 128 | MOTION 64 | LENS 32 | ACCUM 16 | WIDE 8 | HL 4 | SIMPLE 2 | LDS 1.

This module pins the 24 with none of the five feature bits (ALL_KEYS) to the C oracle.  The others belong to the sweeps of
test_lens.py (24), test_motion.py (48), test_medium_layers.py (64), test_solid_gpu.py (128) and test_quad_gpu.py (64), each
compared with the plain-Python restatement; tests/test_feature_matrix.py accounts for all 352.

One small scene per (HL, SIMPLE, table form) cell, through:
  - the one-shot frame against oracle.render (tests/parity.py's bar) and its path count;
  - rt_hip_accumulate over [0, 3) + [3, 7) and [2^20, 2^20 + 4), word for word against oracle.accumulate at the same indices,
    resolved against the oracle's words resolved, and [0, 7) resolved bit for bit against the one-shot frame of 7 samples;
  - (wide cells) the frame and the words of the same scene through the packed tables, bit for bit;
  - rt_hip_accumulate_tiles over a strided, reversed tile list with out-of-range ids: the listed tiles are the whole-frame
    words bit for bit, the others keep their guard words;
  - (a lit and a wide cell) the adaptive host form: each tile is the one-shot frame at the tile's count.
The last test asserts that all 24 base instantiations were launched, so a change that re-routes a cell cannot shrink the coverage
unnoticed."""
import json
import os

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch  # noqa: F401
except ImportError:
    torch = None

from fuzz_worlds import big_flat_world_json
from parity import LINEAR_ATOL, assert_parity, pooled_atol
from test_adaptive import GUARD, _dev, _host, _tiles_match_one_shot, tile_view
from test_progressive import _accumulate, _assert_identical, _new_accum, _one_shot, _resolve, _stream
from test_progressive_reference import _check_words, _resolve_ref, _words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")

W, H, DEPTH = 45, 30, 8          # (neither side a multiple of 4: partial tiles at the right and bottom edges)
N = 7                            # samples of the one-shot frame = [0, 3) + [3, 7)
SPLIT = ((0, 3), (3, N))
HIGH = ((1 << 20), 4)            # (begin, count) of the range high in the index space
LIGHT = {"center": {"x": 0.0, "y": 30.0, "z": 10.0}, "radius": 8.0, "material": {"Light": {}}}
HOT = {"Lambertian": {"albedo": [1.25, 0.6, 0.4]}}   # the ground above 1 in red: the general colour map (rt_tables.h simple_colour)
N_FLAT = 5000                    # a flat world whose tables exceed LDS_TABLES_MAX_BYTES (156 KB) twice over and stay packed (< 65 536 spheres)

FORMS = ("lds", "l2", "wide")
CELLS = [(hl, simple, form) for form in FORMS for hl in (False, True) for simple in (True, False)]
ACCUM, WIDE, HL, SIMPLE, LDS = 16, 8, 4, 2, 1
ALL_KEYS = {k for k in range(32) if not (k & WIDE and k & LDS)}   # (wide tables are never staged in LDS)
SEEN = {}   # last_kernel value -> the first launch that reported it


def _key(hl, simple, form):
    return (WIDE if form == "wide" else 0) | (HL if hl else 0) | (SIMPLE if simple else 0) | (LDS if form == "lds" else 0)


def _key_name(k):
    if k < 0:
        return "none"
    return "<" + ", ".join(f"{n}={int(bool(k & b))}" for n, b in (("HL", HL), ("SIMPLE", SIMPLE), ("LDS", LDS), ("WIDE", WIDE), ("ACCUM", ACCUM))) + ">"


def _cell_id(cell):
    hl, simple, form = cell
    return f"{'lit' if hl else 'unlit'}-{'simple' if simple else 'general'}-{form}"


def _cell_json(hl, simple, form, width=W, height=H, spp=N):
    """lds / wide: the cover scene (484 spheres; wide: RT_GRID_WIDE=1 through the probe library); l2: a flat world of N_FLAT spheres"""
    if form == "l2":
        cfg = json.loads(big_flat_world_json(N_FLAT, np.random.default_rng(11), width=width, height=height, spp=spp, depth=DEPTH, half=35.0))
    else:
        with open(COVER) as f:
            cfg = json.load(f)
        cfg.update(width=width, height=height, samples_per_pixel=spp, max_depth=DEPTH)
    if hl:
        cfg["objects"].append(LIGHT)
    if not simple:
        cfg["objects"][0]["material"] = HOT
    return json.dumps(cfg)


def _open(pkg, host, monkeypatch, cell, **kw):
    """(host scene, resident scene) of a cell; the wide cells through librt_hip_probe.so with RT_GRID_WIDE=1"""
    hl, simple, form = cell
    sc = host.Scene.loads(_cell_json(hl, simple, form, **kw))
    assert len(sc.lights()) == int(hl)
    library = None
    if form == "wide":
        monkeypatch.setenv("RT_GRID_WIDE", "1")
        library = pkg.hip.probe_lib()
    gs = pkg.hip.HipScene(sc.ptr, 0, library=library)
    assert gs.query("grid_wide") == int(form == "wide"), (_cell_id(cell), gs.query("grid_wide"))
    return sc, gs


def _launched(gs, want, what):
    """the last launch of gs ran instantiation `want`; record it for the matrix guard"""
    got = gs.query("last_kernel")
    assert got == want, f"{what}: last_kernel {got} {_key_name(got)}, expected {want} {_key_name(want)}"
    SEEN.setdefault(got, what)


def _check_form(gs, form, what):
    """where the last launch put the tables: asserted, not inferred from a sphere count"""
    assert gs.query("lds_tables") == int(form == "lds"), (what, gs.query("lds_tables"), gs.query("table_bytes"))
    assert gs.query("grid_wide") == int(form == "wide"), (what, gs.query("grid_wide"))


def _list_launch(torch, gs, whole, ranges, want_key, what):
    """rt_hip_accumulate_tiles over every third tile, reversed, plus ids past the grid: the listed tiles must hold `whole`'s words
    (the same ranges accumulated over the whole frame) bit for bit, the others their guard words (test_adaptive.py's check)"""
    grid = gs.tile_grid()
    tw, th, tx, ty = grid
    nt = tx * ty
    assert tx == -(-gs.width // tw) and ty == -(-gs.height // th), (grid, gs.width, gs.height)
    listed = np.arange(1, nt, 3, dtype=np.uint32)
    ids = np.concatenate([listed[::-1], np.array([nt, nt + 7, 0xFFFFFFFF], np.uint32)])[:nt]   # (out-of-range ids are skipped)
    listed = np.array([t for t in ids if t < nt], np.uint32)
    assert 0 < len(listed) < nt
    guard = np.full((gs.height, gs.width, 3), GUARD, np.uint64)
    for t in listed:
        tile_view(guard, t, grid)[...] = 0
    acc = _dev(torch, guard)
    d_list = _dev(torch, ids)
    for b, e in ranges:
        gs.accumulate_tiles(d_list.data_ptr(), len(ids), acc.data_ptr(), b, e - b, None, _stream(torch))
        gs.wait()
        _launched(gs, want_key, f"{what}: list launch [{b}, {e})")
    got = _host(acc, np.uint64)
    want = np.full_like(guard, GUARD)
    for t in listed:
        tile_view(want, t, grid)[...] = tile_view(whole, t, grid)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} words differ (grid {grid})"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_cell_against_the_oracle(pkg, abi, oracle, host, torch_cuda, monkeypatch, cell):
    torch = torch_cuda
    hl, simple, form = cell
    key, name = _key(*cell), _cell_id(cell)
    sc, gs = _open(pkg, host, monkeypatch, cell)
    assert gs.query("last_kernel") == -1   # (scene creation prepares the default configuration; it launches nothing)

    # one-shot
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    rgb, lin, st = _one_shot(torch, gs, N, abi=abi)
    _launched(gs, key, f"{name} one-shot")
    _check_form(gs, form, name)
    assert_parity(rgb, lin, o_rgb, o_lin, f"{name} one-shot", atol=pooled_atol(N))
    assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (name, st["segments"], o_st)
    assert (o_lin > 0).mean() > 0.5 and o_st["segments"] > st["samples"], name   # (a picture, with bounces)
    if hl:
        assert o_st["segments_discarded"] > 0, name    # (light rays were traced)

    # accumulating: two uneven passes, one at a non-zero base
    acc = _new_accum(torch, gs)
    counts = _accumulate(torch, gs, acc, SPLIT)
    _launched(gs, ACCUM | key, f"{name} accumulate {SPLIT}")
    _check_form(gs, form, name)
    words = _words(acc)
    want, ost = oracle.accumulate(abi, sc.ptr, 0, N)
    _check_words(words, want, N, f"{name} [0, {N})")
    assert counts["segments"] == ost["segments"] - ost["segments_discarded"], (name, counts, ost)
    got = _resolve(torch, gs, acc, N)
    _assert_identical(got, (rgb, lin), f"{name}: [0, 3) + [3, {N}) resolved vs the one-shot frame")
    w_rgb, w_lin = _resolve_ref(want.ravel(), N)
    assert_parity(got[0], got[1], w_rgb.reshape(got[0].shape), w_lin.reshape(got[1].shape), f"{name} resolved [0, {N})", atol=LINEAR_ATOL)

    # accumulating: a range high in the index space
    b, c = HIGH
    acc_hi = _new_accum(torch, gs)
    c_hi = _accumulate(torch, gs, acc_hi, ((b, b + c),))
    _launched(gs, ACCUM | key, f"{name} accumulate [{b}, {b + c})")
    want_hi, ost_hi = oracle.accumulate(abi, sc.ptr, b, c)
    _check_words(_words(acc_hi), want_hi, c, f"{name} [{b}, {b + c})")
    assert c_hi["segments"] == ost_hi["segments"] - ost_hi["segments_discarded"], (name, c_hi, ost_hi)
    h_rgb, h_lin = _resolve(torch, gs, acc_hi, c)
    r_rgb, r_lin = _resolve_ref(want_hi.ravel(), c)
    assert_parity(h_rgb, h_lin, r_rgb.reshape(h_rgb.shape), r_lin.reshape(h_lin.shape), f"{name} resolved [{b}, {b + c})", atol=LINEAR_ATOL)

    # list launches, over 4x4 tiles (the words do not depend on the tile geometry)
    gs.set_option("tile_log2", 2)
    _list_launch(torch, gs, words, SPLIT, ACCUM | key, name)
    gs.close()

    if form == "wide":   # another encoding of the packed grid: the packed tables' frame and words (from LDS) bit for bit
        packed = pkg.hip.HipScene(sc.ptr, 0)   # (the product library reads nothing from the environment)
        p_one = _one_shot(torch, packed, N, abi=abi)
        _launched(packed, key & ~WIDE | LDS, f"{name}: the packed tables' one-shot")
        _assert_identical(p_one[:2], (rgb, lin), f"{name}: one-shot vs the packed tables'")
        for (b0, e0), mine in ((SPLIT[0][0], SPLIT[-1][1]), words), ((b, b + c), _words(acc_hi)):
            p_acc = _new_accum(torch, packed)
            _accumulate(torch, packed, p_acc, SPLIT if b0 == 0 else ((b0, e0),))
            _launched(packed, ACCUM | key & ~WIDE | LDS, f"{name}: the packed tables' accumulate")
            p_words = _words(p_acc)
            assert np.array_equal(mine, p_words), f"{name} [{b0}, {e0}): {int((mine != p_words).sum())} words differ from the packed tables'"
        packed.close()


@pytest.mark.parametrize("form", FORMS)
def test_force_lit_renders_the_unlit_frame(pkg, host, torch_cuda, monkeypatch, form):
    """the "force_lit" option sends an unlit scene through the lit kernels (no light to sample): the same frame, the same words
    and the same paths as the unlit kernels"""
    torch = torch_cuda
    cell = (False, True, form)
    key = _key(*cell)
    out = []
    for force in (0, 1):
        sc, gs = _open(pkg, host, monkeypatch, cell)
        gs.set_option("force_lit", force)
        want_key = key | (HL if force else 0)
        what = f"{_cell_id(cell)} force_lit {force}"
        one = _one_shot(torch, gs, N, abi=pkg.abi)
        _launched(gs, want_key, what)
        _check_form(gs, form, what)
        acc = _new_accum(torch, gs)
        counts = _accumulate(torch, gs, acc, SPLIT)
        _launched(gs, ACCUM | want_key, what)
        out.append((one, _words(acc), counts))
        gs.close()
    (one0, w0, c0), (one1, w1, c1) = out
    _assert_identical(one1[:2], one0[:2], f"{form}: force_lit one-shot")
    assert one1[2]["segments"] == one0[2]["segments"], form
    assert np.array_equal(w1, w0), f"{form}: force_lit words differ at {int((w1 != w0).sum())} values"
    assert c1["segments"] == c0["segments"], form


ADAPTIVE_CELLS = [(True, False, "l2"), (True, True, "wide")]


@pytest.mark.parametrize("cell", ADAPTIVE_CELLS, ids=_cell_id)
def test_adaptive_host_form_tiles_are_one_shot_frames(pkg, abi, host, torch_cuda, monkeypatch, cell):
    """rt_hip_render_adaptive_to_host with min_spp 4 of 16 and a threshold between the tiles' round-0 errors (computed here through
    rt_hip_tile_error): the tiles below it stop at 4 samples, the rest are refined, and every tile is the one-shot frame at its count"""
    torch = torch_cuda
    key, name = _key(*cell), _cell_id(cell)
    n, m = 16, 4
    sc, gs = _open(pkg, host, monkeypatch, cell, spp=n)
    ref = pkg.hip.HipScene(sc.ptr, 0, library=pkg.hip.probe_lib() if cell[2] == "wide" else None)
    grid = gs.tile_grid()
    nt = grid[2] * grid[3]
    # round 0 of the host form, restated: [0, m / 2) and [0, m), the error between them
    prev, now = _new_accum(torch, gs), _new_accum(torch, gs)
    _accumulate(torch, gs, prev, ((0, m // 2),))
    _accumulate(torch, gs, now, ((0, m // 2), (m // 2, m)))
    err_dev = _dev(torch, np.full(nt, -1.0, np.float64))
    d_all = _dev(torch, np.arange(nt, dtype=np.uint32))
    gs.tile_error(d_all.data_ptr(), nt, now.data_ptr(), m, prev.data_ptr(), m // 2, err_dev.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    err = _host(err_dev, np.float64)
    u = np.unique(err)
    assert len(u) >= 2 and (err >= 0).all(), (name, u[:4])
    threshold = float(u[len(u) // 2])
    img, n_t, st = gs.render_adaptive(threshold, m)
    _launched(gs, ACCUM | key, f"{name} adaptive")
    assert np.array_equal(n_t.reshape(-1) == m, err < threshold), f"{name}: the tiles that stopped at {m} are not those below the threshold"
    assert n_t.max() > m and set(np.unique(n_t)) <= {m, 2 * m, 4 * m}, (name, np.unique(n_t))
    _tiles_match_one_shot(torch, abi, ref, img, n_t, grid, what=name)
    _launched(ref, key, f"{name} adaptive reference")
    gs.close()
    ref.close()


def test_every_instantiation_was_launched(pkg, host, torch_cuda, monkeypatch):
    """All 24 instantiations were launched, each by the cell that should reach it.  The tests above record what they launched;
    a cell none of them ran (a selection of this module) gets one tiny one-shot and accumulating launch here."""
    torch = torch_cuda
    for cell in CELLS:
        key = _key(*cell)
        if key in SEEN and (ACCUM | key) in SEEN:
            continue
        sc, gs = _open(pkg, host, monkeypatch, cell, width=9, height=6, spp=1)
        _one_shot(torch, gs, 1, abi=pkg.abi)
        _launched(gs, key, f"{_cell_id(cell)} guard one-shot")
        _accumulate(torch, gs, _new_accum(torch, gs), ((0, 1),))
        _launched(gs, ACCUM | key, f"{_cell_id(cell)} guard accumulate")
        gs.close()
    missing = sorted(ALL_KEYS - set(SEEN))
    assert not missing, "instantiations never launched: " + ", ".join(f"{k} {_key_name(k)}" for k in missing)
    assert set(SEEN) == ALL_KEYS, sorted(set(SEEN) - ALL_KEYS)
    print("\nlast_kernel values seen:\n" + "\n".join(f"  {k:2d} {_key_name(k)}: {SEEN[k]}" for k in sorted(SEEN)))
