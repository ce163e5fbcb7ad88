"""Images on flat primitives on the GPU, through the C ABI: 48 x 32 frames at spp 4 against the restatement
(tests/flat_image_mini.py), against "variant" 1 and the scan against the structure bit for bit; the device form of the lookup against
the host build on the CPU test's tables; all 64 QUADS megakernels with one textured entry each; the state — set, remove, set twice, device
memory, updates, passes, shards, adaptive frames, the group, every refusal; the constant-image identity; the CLI."""
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

import flat_image_frames as IF
import flat_image_mini as IM
import flat_image_points as IP
import flat_image_sim as IS
from parity import assert_parity, pooled_atol
from test_medium_gpu import _load, _one_shot, _same, _stream

LDS, SIMPLE, HL, WIDE, ACCUM, LENS, MOTION, MEDIUM, SOLID, QUADS = (1 << b for b in range(10))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
EARTH = os.path.join(ROOT, "scenes", "data", "earth.jpg")
W, H, SPP = IF.W, IF.H, IF.SPP
NONE = 0xFFFFFFFF
TABLES = ("quads", "quad_lim", "flat_bvh", "flat_bvh_order", "flat_normals", "flat_motion", "motion", "flat_lights", "flat_images", "lights", "mat", "matc", "geom")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _scene(pkg, w, bvh=False, images="own", library=None):
    gs = pkg.hip.HipScene(w["sc"].ptr, 0, library=library, center1=w["c1"], quads=w["quads"], flat_bvh=bvh)
    if w["lens"]:
        gs.set_lens(*w["lens"])
    if w["normals"] is not None:
        gs.set_flat_normals(w["normals"])
    images = w["images"] if images == "own" else images
    if images is not None:
        gs.set_flat_images(images)
    if w["emit"] is not None:
        gs.set_flat_lights(w["emit"])
    if w["move"] is not None:
        gs.set_flat_motion(w["move"])
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


def _n_images(w):
    return sum(im.tex_id != NONE for im in w["images"])


def _image_bytes(images):
    return np.frombuffer(bytes(images), np.uint8).reshape(-1, 64).copy()


# ------------------------------------------------------------------ frames against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("case", IF.PARITY_CASES)
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against FlatImageMini; the kernel key is the one of
    the scene without images; "variant" 1 and the structure of §22 give the same frame bit for bit; the first-hit records are the
    restatement's in every bit; RtStats.tex_oob stays 0"""
    w = IF.world(host, abi, case)
    gs = _scene(pkg, w, images=None)
    plain = _one_shot(torch, gs)
    key = gs.query("last_kernel")
    assert gs.query("flat_images") == 0 and gs.table("flat_images") == b""
    gs.set_flat_images(w["images"])
    assert gs.query("flat_images") == _n_images(w) > 0 and len(gs.table("flat_images")) == 64 * len(w["quads"])
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key and key & QUADS and st["tex_oob"] == 0
    assert _differs((rgb, lin), plain), "the images changed nothing"
    m = IF.mini_frame(oracle, abi, host, case)
    print(f"{case}: max |linear diff| {float(np.abs(lin - m['lin']).max()):.3g}, segments gpu {st['segments']} mini {m['segments']} - {m['discarded']}")
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(SPP))
    assert st["segments"] == m["segments"] - m["discarded"]
    gs.set_option("variant", 1)
    _frames_equal((rgb, lin, st), _one_shot(torch, gs), "variant 1")
    assert gs.query("last_kernel") == key
    gs.set_option("variant", 0)
    tree = _scene(pkg, w, bvh=True)
    _frames_equal((rgb, lin, st), _one_shot(torch, tree), "the structure")
    assert tree.query("flat_bvh") > 0 and tree.query("last_kernel") == key and tree.table("flat_images") == gs.table("flat_images")
    tree.close()
    if case in ("poster", "moving_quad", "image_and_emit"):
        want = IF.mini(oracle, abi, w).aovs(SPP)
        got = _aovs(gs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    gs.close()


# ------------------------------------------------------------------ the device form
@pytest.mark.gpu
@pytest.mark.parametrize("cls", IP.CLASSES)
def test_device_texel_against_the_host_build_bit_for_bit(pkg, abi, torch_cuda, cls):
    """rt_hip_flat_image_texel_probe: rt_flat_image.h compiled for the device on the CPU test's class tables (10^5 hits each) against the
    host build of the same header, every bit of col, row and the index, in workgroups of 192 and of 100"""
    rec, ouvw, P = IP.table(cls)
    want = IS.load(abi).texel(rec, ouvw, P)
    L = pkg.hip.probe_lib()
    L.rt_hip_flat_image_texel_probe.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p]
    d_rec = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to("cuda:0")
    d_f = torch.from_numpy(ouvw).to("cuda:0")
    d_P = torch.from_numpy(P).to("cuda:0")
    n = len(rec)
    assert n % 64 != 0 or n == 100_000
    for block in (192, 100):
        d_out = torch.full((n + 8, 3), -7, dtype=torch.int32, device="cuda:0")          # (eight guard rows behind the table)
        pkg.hip._check(L.rt_hip_flat_image_texel_probe(d_rec.data_ptr(), d_f.data_ptr(), d_P.data_ptr(), d_out.data_ptr(), n, block, _stream(torch)), L)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[n:] == -7).all(), "the probe wrote past its table"
        bad = (got[:n].view(np.uint32) != want).any(axis=1)
        assert not bad.any(), (cls, block, int(bad.sum()), got[:n][bad][:2], want[bad][:2])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["poster", "smooth_mesh", "moving_quad"])
def test_device_image_probe_against_the_restatement(pkg, abi, host, torch_cuda, case):
    """rt_hip_flat_image_probe: what the arm in lane_shade runs — the header slot, the entry's resident record and frame, the fetch from the
    resident texels — on 10 007 hits spread over every entry, the origin the entry's Q shifted as a shutter time would shift it, against
    the restatement's colour; an entry without an image answers (-1, 0, 0), an index past the entries NaN; again after update_flats"""
    import quad_mini as QM
    w = IF.world(host, abi, case)
    L = pkg.hip.probe_lib()
    L.rt_hip_flat_image_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    gs = _scene(pkg, w, library=L)
    quads, n_q = w["quads"], len(w["quads"])
    rng = np.random.default_rng(43)
    n = 10007
    k = rng.integers(0, n_q + 1, n).astype(np.uint32)                    # (n_q itself: past the entries)
    kk = np.minimum(k, n_q - 1)
    ab = rng.uniform(-0.1, 1.1, (n, 2))
    shift = rng.uniform(-0.5, 0.5, (n, 3)) * (rng.integers(0, 2, (n, 1)) == 1)
    tex = IF.texture_arrays()
    table = IM.tex_table([(a.shape[1], a.shape[0], a.size) for a in tex])

    def expect(quv):
        origin = quv[kk, 0:3] + shift
        P = origin + quv[kk, 3:6] * ab[:, 0:1] + quv[kk, 6:9] * ab[:, 1:2]
        consts = [QM.QuadConsts(r[0:3], r[3:6], r[6:9]) for r in quv]
        want = np.full((n, 3), np.nan, np.float32)
        for i in range(n):
            if k[i] >= n_q:
                continue
            im = w["images"][int(k[i])]
            code, rec = IM.prepare(list(im.uv), im.tex_id, im.wrap_s, im.wrap_t, im.reserved, table, quads[int(k[i])].kind)
            if code != IM.PRESENT:
                want[i] = (-1.0, 0.0, 0.0)
                continue
            c = consts[int(k[i])]
            index = IM.texel(rec, tuple(origin[i]), c.u, c.v, c.w, tuple(P[i]))[2]
            want[i] = IM.colour(tex[im.tex_id].reshape(-1), index - table[im.tex_id][0])
        return origin, P, want

    def probe(origin, P):
        d_k = torch.from_numpy(k.view(np.int32)).to("cuda:0")
        d_o, d_P = torch.from_numpy(np.ascontiguousarray(origin)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(P)).to("cuda:0")
        d_out = torch.full((n + 8, 3), -7.0, dtype=torch.float32, device="cuda:0")
        pkg.hip._check(L.rt_hip_flat_image_probe(gs._h, d_k.data_ptr(), d_o.data_ptr(), d_P.data_ptr(), d_out.data_ptr(), n, _stream(torch)), L)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[n:] == -7.0).all(), "the probe wrote past its table"
        return got[:n]
    quv = _quv(quads)
    origin, P, want = expect(quv)
    got = probe(origin, P)
    assert np.isnan(got[k >= n_q]).all() and (want[:, 0] >= 0).sum() > n // 20 and (want[:, 0] == -1).sum() > 100
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
    moved = quv.copy()
    moved[:, 0:3] += (0.3, -0.2, 0.1)
    moved[:, 3:6] *= 1.25
    gs.update_flats(moved)
    origin2, P2, want2 = expect(moved)
    got2 = probe(origin2, P2)
    assert np.array_equal(got2.view(np.uint32), want2.view(np.uint32))
    gs.close()


# ------------------------------------------------------------------ every QUADS megakernel
def _sweep_cells():
    import test_quad_gpu as QG
    return QG.SWEEP_CELLS


@pytest.mark.gpu
@pytest.mark.parametrize("cell", range(32))
def test_all_quads_kernels_with_one_textured_entry(pkg, abi, oracle, host, torch_cuda, cell):
    """a cell of test_quad_gpu's sweep with the front face of its box made Lambertian and given an image: the cell reports its key, its
    accumulating twin that key with ACCUM — over the 32 cells the 64 QUADS instantiations — the frame is the restatement's at the parity
    bar with the exact segment count, the passes are the one-shot frame and the grid walk is the full scan, bit for bit"""
    import test_quad_gpu as QG
    cell = QG.SWEEP_CELLS[cell]
    name = QG.sweep_name(cell)
    sc, c1, lens, quads = QG.sweep_world(host, cell, 36, 24)
    keep = IF.attach(abi, sc)
    quads[1].kind = abi.RT_MAT_LAMBERTIAN                               # the box's front face (the floor, then front, right, ...)
    quads[1].albedo[:] = (0.5, 0.5, 0.5)
    images = (abi.RtFlatImage * len(quads))(*[abi.flat_image() for _ in quads])
    images[1] = abi.flat_image(1, (-0.5, 0.0, 1.5, 0.0, -0.5, 1.0), abi.RT_WRAP_REPEAT, abi.RT_WRAP_CLAMP)
    w = {"sc": sc, "c1": c1, "lens": lens, "quads": quads, "normals": None, "move": None, "emit": None, "images": images, "keep": keep}
    gs = _scene(pkg, w)
    want = QG.sweep_key(cell)
    one = _one_shot(torch, gs)
    assert gs.query("last_kernel") == want and gs.query("flat_images") == 1, (name, gs.query("last_kernel"), want)
    mini = IF.mini(oracle, abi, w)
    m_rgb, m_lin, m_segs = mini.render()
    assert mini.image_hits.get(1, 0) > 10, (name, mini.image_hits)
    assert_parity(one[0], one[1], m_rgb, m_lin, name, atol=pooled_atol(2))
    assert one[2]["segments"] == m_segs - mini.discarded, name
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((1, 2), (0, 1)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
    assert gs.query("last_kernel") == want | ACCUM, (name, gs.query("last_kernel"))
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), 2, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), f"{name}: accumulated vs one-shot")
    assert segs == one[2]["segments"], name
    gs.set_option("variant", 1)
    _frames_equal(one, _one_shot(torch, gs), f"{name}: variant 1")
    gs.close()


def test_the_sweep_covers_the_64_quads_kernels():
    import test_quad_gpu as QG
    assert len(QG.SWEEP_CELLS) == 32
    assert {QG.sweep_key(c) | a for c in QG.SWEEP_CELLS for a in (0, ACCUM)} == QG.SWEEP_KEYS and len(QG.SWEEP_KEYS) == 64


# ------------------------------------------------------------------ state
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_set_and_remove(pkg, abi, host, torch_cuda, bvh):
    """images set and then removed (all RT_FLAT_IMAGE_NONE, or NULL): tables byte for byte and frames bit for bit those of a scene that never
    had the call, with the same kernel key; with images only the image table differs; set twice replaces the whole table; device memory"""
    w = IF.world(host, abi, "poster")
    never = _scene(pkg, w, bvh, images=None)
    gs = _scene(pkg, w, bvh)
    want_t, want_f, key = _tables(never), _one_shot(torch, never), never.query("last_kernel")
    shown = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key and _differs(shown, want_f)
    got_t = _tables(gs)
    for name in TABLES:
        if name != "flat_images":
            assert got_t[name] == want_t[name], name
    rec = np.frombuffer(got_t["flat_images"], IS.REC)
    assert want_t["flat_images"] == b"" and len(rec) == len(w["quads"])
    for k, im in enumerate(w["images"]):
        if im.tex_id == NONE:
            assert not np.frombuffer(rec[k].tobytes(), np.uint8).any()
        else:
            off, Wd, Hd = [(0, 8, 4), (32, 5, 3), (47, 1, 1)][im.tex_id]
            assert (rec[k]["texel_off"], rec[k]["W"], rec[k]["H"], rec[k]["wrap"]) == (off, Wd, Hd, im.wrap_s | im.wrap_t << 1)
            assert rec[k]["uv"].tobytes() == bytes(im)[:48]
    none = (abi.RtFlatImage * len(w["quads"]))(*[abi.flat_image() for _ in w["quads"]])
    none[3].uv[0] = float("nan"); none[3].reserved = 9                 # (the rest of an entry without an image is ignored)
    gs.set_flat_images(none)
    assert gs.query("flat_images") == 0 and _tables(gs) == want_t
    _frames_equal(_one_shot(torch, gs), want_f, "all RT_FLAT_IMAGE_NONE")
    assert gs.query("last_kernel") == key
    never.set_flat_images(none)                                        # ... and on a scene that never had any: nothing to do
    assert _tables(never) == want_t
    other = (abi.RtFlatImage * len(w["quads"]))(*none)
    other[3] = abi.flat_image()
    other[4] = abi.flat_image(2)                                       # the right wall, one texel
    gs.set_flat_images(w["images"])
    gs.set_flat_images(other)
    fresh = _scene(pkg, w, bvh, images=other)
    assert _tables(gs) == _tables(fresh) and gs.query("flat_images") == 1
    _frames_equal(_one_shot(torch, gs), _one_shot(torch, fresh), "set twice")
    gs.set_flat_images(torch.from_numpy(_image_bytes(w["images"])).to("cuda:0"))      # ... and back, from device memory
    assert _tables(gs) == got_t
    _frames_equal(_one_shot(torch, gs), shown, "from a tensor")
    gs.set_flat_images(None)
    assert _tables(gs) == want_t
    _frames_equal(_one_shot(torch, gs), want_f, "NULL")
    gs.close(); never.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["scan", "refit", "rebuild"])
def test_update_flats_carries_the_image_with_its_entry(pkg, abi, host, torch_cuda, route):
    """rt_hip_scene_update_flats moving and stretching the poster's wall: the (s, t) are relative to the entry's frame, so tables and frame
    are those of a fresh scene created at the new place with the same images — and not the frame before the move"""
    w = IF.world(host, abi, "poster")
    bvh = route != "scan"
    quv1 = _quv(w["quads"])
    quv1[2, 0:3] += (0.4, 0.0, 0.3)
    quv1[2, 3:6] *= 0.7
    gs = _scene(pkg, w, bvh)
    before = _one_shot(torch, gs)
    gs.update_flats(quv1, rebuild=route == "rebuild")
    assert gs.query("flat_images") == _n_images(w)
    fresh = _scene(pkg, dict(w, quads=_with_geometry(w["quads"], quv1)), bvh)
    got, want = _one_shot(torch, gs), _one_shot(torch, fresh)
    a, b = _tables(gs), _tables(fresh)
    for name in ("quads", "quad_lim", "flat_images", "mat", "matc"):
        assert a[name] == b[name], (route, name)
    _frames_equal(got, want, route)
    assert _differs(got, before)
    gs.close(); fresh.close()


@pytest.mark.gpu
def test_the_sibling_calls_keep_the_images(pkg, abi, host, torch_cuda):
    """update_spheres, set_flat_normals, set_flat_motion and set_flat_lights after the images: each result is the scene built in another
    order; removing what was added gives the first frame back"""
    w = IF.world(host, abi, "smooth_mesh")
    gs = _scene(pkg, w)
    first, images_t = _one_shot(torch, gs), gs.table("flat_images")
    sc = w["sc"]
    centres = np.array([list(s.center) for s in sc.c.spheres[:sc.c.n_spheres]])
    moved = centres.copy(); moved[1, 0] += 0.4
    gs.update_spheres(moved)
    assert gs.table("flat_images") == images_t and gs.query("flat_images") == _n_images(w)
    assert _differs(_one_shot(torch, gs), first)
    gs.update_spheres(centres)
    _frames_equal(_one_shot(torch, gs), first, "the spheres back")
    gs.set_flat_normals(None)                                          # a scan scene keeps the header for its images alone
    assert gs.table("flat_images") == images_t and gs.query("flat_normals") == 0
    flat = _scene(pkg, dict(w, normals=None))
    _frames_equal(_one_shot(torch, gs), _one_shot(torch, flat), "normals removed")
    flat.close()
    gs.set_flat_normals(w["normals"])
    _frames_equal(_one_shot(torch, gs), first, "normals back")
    n = len(w["quads"])
    move = np.zeros((n, 3)); move[2] = (0.3, 0.0, 0.0)
    emit = np.zeros((n, 3), np.float32); emit[1] = (1.0, 0.9, 0.8)
    gs.set_flat_motion(move)
    gs.set_flat_lights(emit)
    assert gs.table("flat_images") == images_t
    other = _scene(pkg, dict(w, move=move, emit=emit))
    _frames_equal(_one_shot(torch, gs), _one_shot(torch, other), "motion and lights after the images")
    assert gs.query("last_kernel") == other.query("last_kernel") and gs.query("last_kernel") & MOTION
    other.close()
    gs.set_flat_lights(None)
    gs.set_flat_motion(None)
    _frames_equal(_one_shot(torch, gs), first, "both removed")
    gs.set_flat_images(None)                                           # the normals keep the header; the images' slots are null again
    bare = _scene(pkg, w, images=None)
    assert _tables(gs) == _tables(bare)
    _frames_equal(_one_shot(torch, gs), _one_shot(torch, bare), "images removed under normals")
    gs.close(); bare.close()


@pytest.mark.gpu
def test_passes_shards_and_adaptive_frames(pkg, abi, host, torch_cuda):
    w = IF.world(host, abi, "poster")
    gs = _scene(pkg, w)
    one = _one_shot(torch, gs)
    key = gs.query("last_kernel")
    acc = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") == key | ACCUM
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
    w = IF.world(host, abi, "metal_fuzz")
    one = _scene(pkg, w)
    want = _one_shot(torch, one)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(w["sc"].ptr, 2, quads=w["quads"])
    monkeypatch.delenv("RT_GPUS_EMULATE")
    try:
        assert grp.size == 2
        plain, _ = grp.render_to_host()
        assert not np.array_equal(plain, want[0])
        bad = (abi.RtFlatImage * len(w["quads"]))(*w["images"])
        bad[1].wrap_t = 2
        with pytest.raises(pkg.host.RtError) as e:
            grp.set_flat_images(bad)
        assert "quad 1:" in str(e.value) and np.array_equal(grp.render_to_host()[0], plain)
        grp.set_flat_images(w["images"])
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])       # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want[0]) and st["segments"] == want[2]["segments"]
        grp.set_flat_images(None, len(w["quads"]))
        assert np.array_equal(grp.render_to_host()[0], plain)
    finally:
        grp.close(); one.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(pkg, abi, host, torch_cuda):
    w = IF.world(host, abi, "poster")
    L = pkg.hip.lib()
    n = len(w["quads"])
    for bvh in (False, True):
        gs = _scene(pkg, w, bvh)
        before, tables = _one_shot(torch, gs), _tables(gs)

        def refused(needle, edit=None, count=None, flags=0, device=False):
            arr = (abi.RtFlatImage * n)(*w["images"])
            if edit:
                edit(arr)
            keep = torch.from_numpy(_image_bytes(arr)).to("cuda:0") if device else arr
            ptr = keep.data_ptr() if device else C.addressof(arr)
            with pytest.raises(pkg.host.RtError) as e:
                pkg.hip._check(L.rt_hip_scene_set_flat_images(gs._h, ptr, n if count is None else count, flags | (abi.RT_UPDATE_FLATS_DEVICE if device else 0)), L)
            assert e.value.code == abi.RT_ERR_INVALID and needle in str(e.value), str(e.value)
            assert _tables(gs) == tables
            _frames_equal(_one_shot(torch, gs), before, needle)

        def two(a):
            a[7].uv[3] = float("nan"); a[2].tex_id = 3
        for device in (False, True):
            refused("quad 2: tex_id", two, device=device)              # of two bad entries the lowest, with its reason
            refused("quad 0: every uv", lambda a: a[0].uv.__setitem__(5, float("inf")), device=device)
            refused("quad 2: wrap", lambda a: setattr(a[2], "wrap_s", 2), device=device)
            refused("quad 2: reserved", lambda a: setattr(a[2], "reserved", 1), device=device)
        refused("n_quads", count=n - 1)
        refused("unknown flag", flags=4)
        refused("unknown flag", flags=abi.RT_UPDATE_FLATS_REBUILD)
        # a second view of the scene's tables, made the way a group makes its ranks' views (an internal C++ entry point)
        nm = subprocess.run(["nm", "-D", "--defined-only", pkg.hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
        sym = [l.split()[-1] for l in nm.splitlines() if "rt_hip_scene_clone_view" in l]
        assert len(sym) == 1, sym
        clone = getattr(L, sym[0])
        clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        view = C.c_void_p()
        assert clone(gs._h, C.byref(view)) == abi.RT_OK
        try:
            refused("rt_hip_group_set_flat_images")
        finally:
            L.rt_hip_scene_destroy(view)
        gs.set_flat_images(w["images"])                                # ... and once the view is gone the same call goes through
        assert _tables(gs) == tables
        gs.close()
    with pytest.raises(pkg.host.RtError):
        pkg.hip._check(L.rt_hip_scene_set_flat_images(None, None, 0, 0), L)


@pytest.mark.gpu
def test_refused_materials_and_textures(pkg, abi, host, torch_cuda):
    """an image on a Glass or a Checker entry, on a texture whose nbytes is not 3 W H, and in a scene without any texture"""
    import test_quad_gpu as QG
    objs = IF._floor_objs(floor=QG._chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 1.5), extra=[IF._quad((-1.5, -0.5, 3.4), (3, 0, 0.4), (0, 2.2, 0), IF.GLASS)])
    sc, c1, lens = _load(host, IF._cfg(objs), W, H, SPP, 8, seed=3)
    quads = sc.quads()
    gs = pkg.hip.HipScene(sc.ptr, 0, quads=quads)                      # (no texture at all)
    before = _one_shot(torch, gs)
    arr = (abi.RtFlatImage * 3)(abi.flat_image(), abi.flat_image(0), abi.flat_image())
    with pytest.raises(pkg.host.RtError) as e:
        gs.set_flat_images(arr)
    assert "quad 1: tex_id" in str(e.value)
    gs.close()
    tex = IF.texture_arrays()
    tex[1] = tex[1].reshape(-1)[:-3].reshape(1, -1, 3)                  # 14 texels that claim to be ...
    keep = IF.attach(abi, sc, tex)
    keep[0][1].width, keep[0][1].height = 5, 3                         # ... 5 x 3
    gs = pkg.hip.HipScene(sc.ptr, 0, quads=quads)
    for k, tid, needle in ((0, 0, "quad 0: an image needs"), (2, 0, "quad 2: an image needs"), (1, 1, "quad 1: the texture's nbytes")):
        arr = (abi.RtFlatImage * 3)(*[abi.flat_image() for _ in range(3)])
        arr[k] = abi.flat_image(tid)
        with pytest.raises(pkg.host.RtError) as e:
            gs.set_flat_images(arr)
        assert needle in str(e.value), str(e.value)
        assert gs.query("flat_images") == 0
    _frames_equal(_one_shot(torch, gs), before, "refused")
    arr = (abi.RtFlatImage * 3)(abi.flat_image(), abi.flat_image(2), abi.flat_image())      # the third texture starts behind the short one
    gs.set_flat_images(arr)
    assert np.frombuffer(gs.table("flat_images"), IS.REC)[1]["texel_off"] == 32 + 14
    gs.close()


@pytest.mark.gpu
def test_headline_scene_keeps_its_kernel(pkg, abi, load_scene, torch_cuda):
    sc = load_scene("cover", 48, 32, 2)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    _one_shot(torch, gs)
    assert gs.query("last_kernel") == 3 and gs.query("flat_images") == 0 and gs.table("flat_images") == b""
    with pytest.raises(pkg.host.RtError):
        gs.set_flat_images((abi.RtFlatImage * 1)(abi.flat_image()))     # no flat primitive
    gs.close()


# ------------------------------------------------------------------ a check with no restatement
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_constant_image_identity(pkg, abi, host, torch_cuda, bvh):
    """a one-colour image c on a Lambertian wall: the frame and the first-hit records are, bit for bit, those of the scene without images
    whose wall has albedo = c / 255 — a path that never enters the new function"""
    sim = IS.load(abi)
    a, b = IF.constant_pair(host, abi, lambda v: float(sim.colour(np.array([v], np.uint32))[0, 0]))
    ga, gb = _scene(pkg, a, bvh), _scene(pkg, b, bvh)
    fa, fb = _one_shot(torch, ga), _one_shot(torch, gb)
    assert ga.query("flat_images") == 1 and gb.query("flat_images") == 0 and ga.query("last_kernel") == gb.query("last_kernel")
    _frames_equal(fa, fb, "constant image")
    assert np.array_equal(_aovs(ga).view(np.uint32), _aovs(gb).view(np.uint32))
    ga.close(); gb.close()


# ------------------------------------------------------------------ the CLI
def _cli_cfg():
    objs = IF._room_objs()
    objs[2]["image"] = {"pixels": EARTH}
    objs[6]["image"] = {"pixels": os.path.join(ROOT, "scenes", "data", "moon.jpg"), "wrap": "clamp"}
    cfg = IF._room_cfg(objs)
    cfg.update(width=W, height=H, samples_per_pixel=SPP, max_depth=8)
    return cfg


def _strip(cfg):
    cfg = json.loads(json.dumps(cfg))
    for o in cfg["objects"]:
        o.pop("image", None); o.pop("uvs", None)
    return cfg


@pytest.mark.gpu
def test_cli_renders_a_file_with_images(pkg, abi, host, torch_cuda, tmp_path):
    """a small file through `raytracer`: the API frame of the same file byte for byte, and NOT the frame of the file with "image" stripped"""
    from PIL import Image
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    cfg = _cli_cfg()
    imgs = {}
    for name, c in (("shown", cfg), ("plain", _strip(cfg))):
        (tmp_path / f"{name}.json").write_text(json.dumps(c))
        r = subprocess.run([EXE, str(tmp_path / f"{name}.json"), str(tmp_path / f"{name}.png")], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.stdout, r.stderr)
        imgs[name] = np.asarray(Image.open(tmp_path / f"{name}.png").convert("RGB"))
    assert not np.array_equal(imgs["shown"], imgs["plain"]), "the CLI ignored the file's images"
    sc = host.Scene.load(str(tmp_path / "shown.json"))
    gs = pkg.hip.HipScene(sc.ptr, 0, quads=sc.quads())
    gs.set_flat_images(sc.flat_images())
    api, _ = gs.render_to_host()
    assert gs.query("flat_images") == 7
    gs.close()
    assert np.array_equal(api, imgs["shown"])


@pytest.mark.gpu
def test_cli_flat_frames_keep_the_base_files_images(pkg, abi, host, torch_cuda, tmp_path):
    """`--frames 2 --flat-frames PREFIX` with a textured base: the frame files carry geometry only and the images stay — each frame is the
    one-shot render of the base file at that frame's geometry; a frame file that itself carries "image" is refused, naming the file"""
    from PIL import Image
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    base = _cli_cfg()
    (tmp_path / "base.json").write_text(json.dumps(base))

    def at(f, stripped):
        cfg = json.loads(json.dumps(base))
        cfg["objects"][2]["q"]["x"] += 0.3 * f
        return _strip(cfg) if stripped else cfg

    def run(*args, ok=True):
        r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)
        assert (r.returncode == 0) == ok, (args, r.stdout, r.stderr)
        return r
    for f in range(2):
        (tmp_path / f"fr_{f:03d}.json").write_text(json.dumps(at(f, True)))
        (tmp_path / f"want_{f}.json").write_text(json.dumps(at(f, False)))
        run(tmp_path / f"want_{f}.json", tmp_path / f"want_{f}.png")
    run(tmp_path / "base.json", tmp_path / "out", "--frames", 2, "--orbit", 0, "--flat-frames", tmp_path / "fr_")
    img = lambda name: np.asarray(Image.open(tmp_path / name).convert("RGB"))
    for f in range(2):
        assert np.array_equal(img(f"out_{f:03d}.png"), img(f"want_{f}.png")), f
    assert not np.array_equal(img("want_0.png"), img("want_1.png"))
    (tmp_path / "bad_000.json").write_text(json.dumps(at(0, False)))
    (tmp_path / "bad_001.json").write_text(json.dumps(at(1, True)))
    r = run(tmp_path / "base.json", tmp_path / "no", "--frames", 2, "--orbit", 0, "--flat-frames", tmp_path / "bad_", ok=False)
    assert "bad_000.json" in r.stderr + r.stdout and "image" in r.stderr + r.stdout, (r.stdout, r.stderr)
