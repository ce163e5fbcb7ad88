"""The thin-lens camera: the camera map's "aperture" / "focus_dist", rt_camera_derive_lens, rt_hip_set_lens and
the LENS instantiations of the megakernel.

The reference for lens frames is a lens render loop here: tests/mini_oracle.py's ray_color and Philox with only the camera
lines of Mini.render replaced — the lens point by rejection in the unit disc, node NODE_CAMERA, slots 1, 2, ...  Colour is
compared at the project's parity bar (tests/parity.py: the kernel composes colour outermost-first and sums pixels in exact
fixed point); geometry and paths are exact, so unlit path counts are equal."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import mini_oracle as M
from parity import assert_parity, pooled_atol
from test_kernel_matrix import ALL_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")
TEST = os.path.join(ROOT, "scenes", "cfg1_test_800x600_spp16.json")
TEX = os.path.join(ROOT, "scenes", "cfg3_cover_4k_textured.json")
DOF = os.path.join(ROOT, "scenes", "cover_dof_1200x800_spp128.json")
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRT_WAVES_PER_EU=4"]  # build.py's
LENS = 32   # rt_hip_scene_query("last_kernel") bit of the LENS instantiations
SWEEP_KEYS = {LENS | k for k in ALL_KEYS}   # the 24 that test_every_lens_instantiation_is_launched pins


def _cfg(path, **cam):
    with open(path) as f:
        cfg = json.load(f)
    cfg["camera"].update(cam)
    return cfg


def _camera_text(extra):
    """the headline scene's text with `extra` (raw JSON members) added to its camera map"""
    text = open(COVER).read()
    anchor = '"aspect":1.5'
    assert text.count(anchor) == 1
    return text.replace(anchor, anchor + extra)


def _lens_of(host, sc):
    out = (C.c_double * 2)()
    host.lib().rt_scene_lens(sc._h, out)
    return tuple(out)


def _derive_py(lf, la, up, vfov, aspect, aperture, focus):
    """rt_camera_derive_lens restated from the contract (camera.rs:45-77 + the lens): every operation one IEEE f64 operation"""
    def unit(v):
        n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return (v[0] / n, v[1] / n, v[2] / n)

    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    f = 1.0 if aperture == 0.0 else focus
    theta = vfov * (math.pi / 180.0)
    half_height = math.tan(theta / 2.0)
    half_width = aspect * half_height
    hw, hh = half_width * f, half_height * f
    d = (lf[0] - la[0], lf[1] - la[1], lf[2] - la[2])
    w = unit(d)
    u = unit(cross(up, w))
    v = cross(w, u)
    ll = [((lf[i] - u[i] * hw) - v[i] * hh) - w[i] * f for i in range(3)]
    hor = [(u[i] * 2.0) * hw for i in range(3)]
    ver = [(v[i] * 2.0) * hh for i in range(3)]
    return list(lf) + ll + hor + ver + [math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])] + list(u) + list(v) + [aperture / 2.0]


def _bits(xs):
    return np.array(xs, np.float64).view(np.uint64).tolist()


# ---------------------------------------------------------------------------------------------------- no GPU needed

def test_schema_defaults_and_integer_literals(host):
    plain = host.Scene.load(COVER)
    lens = _lens_of(host, plain)
    assert lens[0] == 0.0 and lens[1] == math.sqrt(13.0 ** 2 + 2.0 ** 2 + 3.0 ** 2)   # focus_dist defaults to focal_length
    assert _lens_of(host, host.Scene.load(DOF)) == (0.1, 10.0)
    assert _lens_of(host, host.Scene.loads(_camera_text(',"aperture":1,"focus_dist":7'))) == (1.0, 7.0)
    assert _lens_of(host, host.Scene.loads(_camera_text(',"aperture":0.25')))[1] == lens[1]
    assert _lens_of(host, host.Scene.loads(_camera_text(',"aperture":0,"focus_dist":3'))) == (0.0, 3.0)
    # the camera RtScene carries is the pinhole's whatever the keys (a lens is set on a resident scene)
    for extra in (',"aperture":0.1,"focus_dist":10', ',"aperture":0,"focus_dist":3'):
        sc = host.Scene.loads(_camera_text(extra))
        for f in ("cam_origin", "cam_lower_left", "cam_horizontal", "cam_vertical"):
            assert list(getattr(sc.c, f)) == list(getattr(plain.c, f)), (extra, f)
    # the sequence form of CameraParams stays the reference's five fields
    cfg = json.load(open(COVER))
    c = cfg["camera"]
    cfg["camera"] = [c["look_from"], c["look_at"], c["vup"], c["vfov"], c["aspect"]]
    assert _lens_of(host, host.Scene.loads(json.dumps(cfg)))[0] == 0.0


@pytest.mark.parametrize("extra,msg", [
    (',"aperture":-0.1', "camera.aperture"),
    (',"aperture":-0', None),   # (-0 == 0: the pinhole)
    (',"aperture":1e999', "out of range"),
    (',"aperture":"0.1"', "camera.aperture"),
    (',"aperture":null', "camera.aperture"),
    (',"focus_dist":0', "camera.focus_dist"),
    (',"focus_dist":-2', "camera.focus_dist"),
    (',"aperture":0,"focus_dist":0', "camera.focus_dist"),
    (',"aperture":0.1,"focus_dist":-1e999', "out of range"),
    (',"aperture":0.1,"aperture":0.2', "duplicate field `aperture`"),
    (',"focus_dist":3,"focus_dist":3', "duplicate field `focus_dist`"),
])
def test_schema_errors(host, abi, extra, msg):
    if msg is None:
        assert _lens_of(host, host.Scene.loads(_camera_text(extra)))[0] == 0.0
        return
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_camera_text(extra))
    assert e.value.code == abi.RT_ERR_PARSE and msg in str(e.value), str(e.value)


def test_to_json_writes_the_keys_only_if_the_file_had_them(host):
    base = host.Scene.load(COVER).to_json()
    assert '"aperture"' not in base and '"focus_dist"' not in base and '"aspect":1.5},"objects"' in base
    for extra in (',"aperture":0.1,"focus_dist":10', ',"aperture":0', ',"focus_dist":2.5', ',"aperture":0.5'):
        s = host.Scene.loads(_camera_text(extra)).to_json()
        want = base.replace('"aspect":1.5}', '"aspect":1.5' + extra.replace(":10", ":10.0").replace(":0,", ":0.0,")
                            .replace('"aperture":0', '"aperture":0.0' if extra == ',"aperture":0' else '"aperture":0') + "}")
        assert s == want, (extra, s[s.index('"camera"'):s.index('"objects"')])
        assert host.Scene.loads(s).to_json() == s   # round trip
    dof = host.Scene.load(DOF).to_json()
    assert dof == base.replace('"aspect":1.5}', '"aspect":1.5,"aperture":0.1,"focus_dist":10.0}')


def test_existing_scenes_serialise_without_lens_keys(host):
    for name in ("cfg1_test_800x600_spp16.json", "cfg2_cover_1200x800_spp128.json", "cfg3_cover_4k_textured.json"):
        s = host.Scene.load(os.path.join(ROOT, "scenes", name)).to_json()
        assert '"aperture"' not in s and '"focus_dist"' not in s, name
        cam = json.loads(s)["camera"]
        assert list(cam) == ["look_from", "look_at", "vup", "vfov", "aspect"], name


@pytest.mark.parametrize("case", [
    ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.5, 0.1, 10.0),
    ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.5, 0.0, 3.0),
    ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.5, 0.0, 13.490737563232042),
    ((-3.5, 7.25, 11.0), (0.5, -1.0, 2.0), (0.1, 1.0, -0.2), 47.5, 1.7777777777777777, 2.0, 3.3),
    ((0.0, 0.0, -5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 90.0, 1.0, 1e-6, 1e3),
])
def test_camera_derive_lens_restated_bit_for_bit(host, case):
    got = host.camera_derive_lens(*case)
    flat = got["origin"] + got["lower_left_corner"] + got["horizontal"] + got["vertical"] + [got["focal_length"]] + got["u"] + got["v"] + [got["lens_radius"]]
    assert _bits(flat) == _bits(_derive_py(*case))
    if case[5] == 0.0:   # the pinhole: rt_camera_derive's 13 values, bit for bit, whatever focus_dist
        pin = host.camera_derive(*case[:5])
        want = pin["origin"] + pin["lower_left_corner"] + pin["horizontal"] + pin["vertical"] + [pin["focal_length"]]
        assert _bits(flat[:13]) == _bits(want) and flat[19] == 0.0


# ---------------------------------------------------------------------------------------------------- GPU

class LensMini(M.Mini):
    """Mini.render with the camera lines replaced by the thin lens of the contract"""

    def __init__(self, scene, atan2, u, v, r):
        super().__init__(scene, atan2)
        self.lu, self.lv, self.r = tuple(u), tuple(v), r

    def lens_disc(self):
        a = 0
        while True:
            w = self.words(M.NODE_CAMERA, 1 + a)
            for x, y in ((w[0], w[1]), (w[2], w[3])):
                px, py = M.range_m1_1(x), M.range_m1_1(y)
                if px * px + py * py < 1.0:
                    return px, py
            a += 1

    def camera_ray(self, x, y):
        sc = self.sc
        W, H = sc.width, sc.height
        org, ll, hor, ver = (tuple(v) for v in (sc.cam_origin, sc.cam_lower_left, sc.cam_horizontal, sc.cam_vertical))
        w = self.words(M.NODE_CAMERA, 0)
        u = (float(x) + M.u01_53(w[0], w[1])) / (float(W) - 1.0)
        v = (float(H) - (float(y) + M.u01_53(w[2], w[3]))) / (float(H) - 1.0)
        px, py = self.lens_disc()
        rx, ry = self.r * px, self.r * py
        off = M.add(M.muls(self.lu, rx), M.muls(self.lv, ry))
        d = M.sub(M.sub(M.add(M.add(ll, M.muls(hor, u)), M.muls(ver, v)), org), off)
        return M.add(org, off), d

    def render(self):
        sc = self.sc
        W, H, spp = sc.width, sc.height, sc.samples_per_pixel
        lin, rgb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.uint8)
        for y in range(H):
            for x in range(W):
                acc = [M.F(0.0), M.F(0.0), M.F(0.0)]
                self.pixel = y * W + x
                for s in range(spp):
                    self.sample = s
                    o, d = self.camera_ray(x, y)
                    c = self.ray_color(o, d, sc.max_depth, sc.max_depth, 0, 0)
                    acc = [acc[k] + c[k] for k in range(3)]
                scale = M.F(1.0) / M.F(spp)
                for k in range(3):
                    lin[y, x, k] = scale * acc[k]
                    g = np.sqrt(scale * acc[k]) * M.F(255.0)
                    rgb[y, x, k] = 255 if g != g else int(np.rint(min(max(g, M.F(0.0)), M.F(255.0))))
        return rgb, lin, self.segments


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _lens_scene(host, cfg, w, h, spp, depth=8, seed=None):
    """(host scene with the lens camera in its RtScene fields, (u, v, r)) of a config whose camera map may hold a lens"""
    sc = host.Scene.loads(json.dumps(cfg))
    c = sc.c
    c.width, c.height, c.samples_per_pixel, c.max_depth = w, h, spp, depth
    if seed is not None:
        c.seed = seed
    cam = cfg["camera"]
    pt = lambda p: (float(p["x"]), float(p["y"]), float(p["z"]))
    aperture, focus = _lens_of(host, sc)
    d = host.camera_derive_lens(pt(cam["look_from"]), pt(cam["look_at"]), pt(cam["vup"]), float(cam["vfov"]), float(cam["aspect"]), aperture, focus)
    for i in range(3):
        c.cam_origin[i], c.cam_lower_left[i], c.cam_horizontal[i], c.cam_vertical[i] = (d["origin"][i], d["lower_left_corner"][i],
                                                                                         d["horizontal"][i], d["vertical"][i])
    return sc, (d["u"], d["v"], d["lens_radius"])


def _one_shot(torch, gs, spp=None):
    if spp is not None:
        gs.set_option("samples_per_pixel", spp)
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.render(rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    st = gs.wait()
    return rgb.cpu().numpy(), lin.cpu().numpy(), st


def _accumulated(torch, gs, ranges, n):
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ranges:
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), n, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    return rgb.cpu().numpy(), lin.cpu().numpy(), segs


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: RGB8 differs at {int((a[0] != b[0]).sum())} values"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: linear radiance differs bitwise"


def _mini(oracle, abi, sc, lens):
    L = oracle.lib(abi)
    return LensMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), *lens)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [{"aperture": 0}, {"aperture": 0, "focus_dist": 3}])
def test_zero_aperture_is_the_pinhole_frame(pkg, host, torch_cuda, extra):
    """aperture 0 (with or without focus_dist): the keyless scene's frame, byte for byte, one-shot and accumulated — through
    rt_camera_derive_lens + rt_hip_set_camera + rt_hip_set_lens(r = 0)"""
    torch = torch_cuda
    W, H, N = 37, 23, 5
    ref, _ = _lens_scene(host, _cfg(COVER), W, H, N)
    sc, lens = _lens_scene(host, _cfg(COVER, **extra), W, H, N)
    assert lens[2] == 0.0
    a, b = pkg.hip.HipScene(ref.ptr, 0), pkg.hip.HipScene(sc.ptr, 0)
    b.set_lens(*lens)
    assert b.query("lens") == 0
    want = _one_shot(torch, a)
    got = _one_shot(torch, b)
    _same(got, want, f"{extra} one-shot")
    assert got[2]["segments"] == want[2]["segments"] and b.query("last_kernel") & LENS == 0
    _same(_accumulated(torch, b, ((2, 5), (0, 2)), N), want, f"{extra} accumulated")
    a.close(); b.close()


LENS_CASES = {
    # (scene config, w, h, spp, depth, lens keys): a cover-like world at the book's lens and a wide one focused near, a lit scene
    # (lights, textures, glass), a textured scene with a texture sky
    "cover_book": (COVER, 24, 16, 3, 8, {"aperture": 0.1, "focus_dist": 10.0}),
    "cover_wide_near": (COVER, 24, 16, 3, 8, {"aperture": 0.6, "focus_dist": 4.5}),
    "lit": (TEST, 20, 15, 3, 8, {"aperture": 0.3, "focus_dist": 2.0}),
    "textured": (TEX, 24, 14, 2, 8, {"aperture": 0.4, "focus_dist": 25.0}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LENS_CASES))
def test_lens_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case):
    torch = torch_cuda
    path, w, h, spp, depth, keys = LENS_CASES[case]
    sc, lens = _lens_scene(host, _cfg(path, **keys), w, h, spp, depth)
    assert lens[2] == keys["aperture"] / 2.0
    m_rgb, m_lin, m_segs = _mini(oracle, abi, sc, lens).render()
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.set_lens(*lens)
    assert gs.query("lens") == 1
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") & LENS
    assert_parity(rgb, lin, m_rgb, m_lin, f"{case} one-shot", atol=pooled_atol(spp))
    if gs.query("n_lights") == 0:
        assert st["segments"] == m_segs, (case, st["segments"], m_segs)
    else:   # (the kernel does not trace the light loops raytracer.rs:124 throws away; the restatement does)
        assert 0 < st["segments"] <= m_segs, (case, st["segments"], m_segs)
    # the lens changes the picture: the pinhole frame of the same scene differs
    pin_sc, _ = _lens_scene(host, _cfg(path), w, h, spp, depth)
    pin = pkg.hip.HipScene(pin_sc.ptr, 0)
    assert not np.array_equal(_one_shot(torch, pin)[1], lin)
    gs.close()
    pin.close()


@pytest.mark.gpu
def test_every_lens_instantiation_is_launched(pkg, abi, oracle, host, torch_cuda, monkeypatch):
    """each (lights, simple colour, table form) cell of tests/test_kernel_matrix.py through a lens, one-shot and accumulating:
    the 24 LENS instantiations, each frame at the parity bar against the restatement, the accumulated frame the one-shot's"""
    from test_kernel_matrix import ACCUM, CELLS, _cell_id, _cell_json, _key
    torch = torch_cuda
    seen = {}
    for cell in CELLS:
        hl, simple, form = cell
        name = _cell_id(cell)
        cfg = json.loads(_cell_json(hl, simple, form, width=9, height=6, spp=2))
        cfg["camera"].update(aperture=0.5, focus_dist=7.0)
        sc, lens = _lens_scene(host, cfg, 9, 6, 2)
        library = None
        if form == "wide":
            monkeypatch.setenv("RT_GRID_WIDE", "1")
            library = pkg.hip.probe_lib()
        gs = pkg.hip.HipScene(sc.ptr, 0, library=library)
        monkeypatch.delenv("RT_GRID_WIDE", raising=False)
        gs.set_lens(*lens)
        one = _one_shot(torch, gs)
        k = gs.query("last_kernel")
        assert k == LENS | _key(*cell), (name, k)
        seen.setdefault(k, name)
        acc = _accumulated(torch, gs, ((1, 2), (0, 1)), 2)
        k = gs.query("last_kernel")
        assert k == LENS | ACCUM | _key(*cell), (name, k)
        seen.setdefault(k, name)
        _same(acc, one, f"{name}: accumulated vs one-shot")
        m_rgb, m_lin, m_segs = _mini(oracle, abi, sc, lens).render()
        assert_parity(one[0], one[1], m_rgb, m_lin, name, atol=pooled_atol(2))
        if not hl:
            assert one[2]["segments"] == m_segs == acc[2], (name, one[2]["segments"], m_segs, acc[2])
        gs.close()
    assert set(seen) == SWEEP_KEYS, sorted(set(seen) ^ SWEEP_KEYS)


@pytest.mark.gpu
def test_composition_under_a_lens(pkg, abi, oracle, host, torch_cuda):
    """passes, adaptive tiles, AOVs and the denoised host form compose exactly under a lens, as they do through the pinhole"""
    from test_adaptive import _tiles_match_one_shot
    from test_denoise import _aovs
    torch = torch_cuda
    N = 9
    sc, lens = _lens_scene(host, _cfg(COVER, aperture=0.4, focus_dist=6.0), 40, 24, N)
    gs, ref = pkg.hip.HipScene(sc.ptr, 0), pkg.hip.HipScene(sc.ptr, 0)
    for s in (gs, ref):
        s.set_lens(*lens)
    one = _one_shot(torch, ref)
    # an uneven, out-of-order pass split
    got = _accumulated(torch, gs, ((6, 9), (0, 1), (1, 6)), N)
    _same(got, one, "passes [6, 9) + [0, 1) + [1, 6)")
    assert got[2] == one[2]["segments"]
    # the adaptive host form: tile by tile the one-shot frame at the tile's count
    sc2, _ = _lens_scene(host, _cfg(COVER, aperture=0.4, focus_dist=6.0), 80, 48, 32)
    ad, ad_ref = pkg.hip.HipScene(sc2.ptr, 0), pkg.hip.HipScene(sc2.ptr, 0)
    for s in (ad, ad_ref):
        s.set_lens(*lens)
    img, n_t, _ = ad.render_adaptive(0.05, 8)
    assert len(np.unique(n_t)) > 1, np.unique(n_t)
    _tiles_match_one_shot(torch, abi, ad_ref, img, n_t, ad.tile_grid(), what="lens adaptive")
    ad.close(); ad_ref.close()
    # the AOVs: the restatement's first hit of the same lens ray
    n = 3
    aov = _aovs(torch, gs, n).cpu().numpy()
    m = _mini(oracle, abi, sc, lens)
    want = np.zeros_like(aov)
    W, H = sc.c.width, sc.c.height
    for y in range(H):
        for x in range(W):
            acc = [0.0] * 8
            m.pixel = y * W + x
            for s in range(n):
                m.sample = s
                o, d = m.camera_ray(x, y)
                hit = m.hit_world(o, d)
                if hit is None:
                    alb = m.sky_colour(d)
                else:
                    i, p, nrm, front = hit
                    ob = m.obj[i]
                    alb = (1.0, 1.0, 1.0) if ob.kind in (M.GLASS, M.LIGHT) else tuple(np.float32(a) for a in ob.albedo)
                    t = M.dot(M.sub(p, o), d) / M.len2(d)   # (p = o + t d: the root hit_world accepted, recovered)
                    acc[3] += 1.0 / t
                    acc[4] += nrm[0]; acc[5] += nrm[1]; acc[6] += nrm[2]
                    acc[7] += 1.0
                for k in range(3):
                    acc[k] += float(alb[k])
            want[y, x] = [np.float32(a / float(n)) for a in acc]
    for ch in (0, 1, 2, 4, 5, 6, 7):   # albedo, normal, coverage: exact
        assert np.array_equal(aov[..., ch].view(np.uint32), want[..., ch].view(np.uint32)), ch
    assert np.allclose(aov[..., 3], want[..., 3], rtol=1e-12, atol=0)   # inv_depth: t recovered from the hit point
    # the denoised host form: K passes give the bytes of one
    d1 = pkg.hip.HipScene(sc.ptr, 0)
    d1.set_lens(*lens)
    one_d, _ = d1.refine_to_host_denoised(N)
    for c in (4, 2, 3):
        last, _ = gs.refine_to_host_denoised(c)
    assert gs.query("accum_samples") == N
    assert np.array_equal(last, one_d)
    d1.close(); gs.close(); ref.close()


@pytest.mark.gpu
def test_set_lens_and_set_camera_in_either_order_and_resets(pkg, host, torch_cuda):
    torch = torch_cuda
    W, H, N = 32, 20, 4
    plain, _ = _lens_scene(host, _cfg(COVER), W, H, N)
    sc, lens = _lens_scene(host, _cfg(COVER, aperture=0.5, focus_dist=8.0), W, H, N)
    ref = pkg.hip.HipScene(sc.ptr, 0)
    ref.set_lens(*lens)
    want = _one_shot(torch, ref)
    c = sc.c
    cam = [list(c.cam_origin), list(c.cam_lower_left), list(c.cam_horizontal), list(c.cam_vertical)]
    for order in ("lens_first", "camera_first"):
        gs = pkg.hip.HipScene(plain.ptr, 0)   # (the keyless pinhole scene: both the camera and the lens move)
        if order == "lens_first":
            gs.set_lens(*lens); gs.set_camera(*cam)
        else:
            gs.set_camera(*cam); gs.set_lens(*lens)
        _same(_one_shot(torch, gs), want, order)
        gs.close()
    # a lens change starts the accumulator over; the same lens again does not
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.set_lens(*lens)
    gs.refine_to_host(2)
    assert gs.query("accum_samples") == 2
    gs.set_lens(*lens)
    assert gs.query("accum_samples") == 2
    gs.set_lens(lens[0], lens[1], lens[2] * 0.5)
    assert gs.query("accum_samples") == 0
    gs.refine_to_host(1)
    gs.set_lens(lens[0], lens[1], 0.0)
    assert gs.query("accum_samples") == 0 and gs.query("lens") == 0
    # bad radii are refused and change nothing
    gs.set_lens(*lens)
    gs.refine_to_host(2)
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(pkg.host.RtError) as e:
            gs.set_lens(lens[0], lens[1], bad)
        assert e.value.code == pkg.abi.RT_ERR_INVALID
        assert gs.query("accum_samples") == 2 and gs.query("lens") == 1
    _same(_one_shot(torch, gs), want, "after refused radii")
    gs.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_group_lens_frame_is_the_single_gpu_frame(pkg, host, torch_cuda, world):
    torch = torch_cuda
    sc, lens = _lens_scene(host, _cfg(TEST, aperture=0.3, focus_dist=2.0), 64, 49, 3)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.set_lens(*lens)
    want = _one_shot(torch, gs)
    gs.close()
    os.environ["RT_GPUS_EMULATE"] = "1"
    try:
        grp = pkg.hip.HipGroup(sc.ptr, world)
    finally:
        del os.environ["RT_GPUS_EMULATE"]
    assert grp.size == world
    grp.set_lens(*lens)
    for _ in range(2):
        got, st = grp.render_to_host()
        assert np.array_equal(got, want[0]) and st["segments"] == want[2]["segments"]
    grp.close()


def _orbit_py(cam, lens, deg, f, host):
    """main.cpp orbit_camera restated (Rodrigues about vup, then rt_camera_derive_lens)"""
    lf, la, up = cam[0:3], cam[3:6], cam[6:9]
    kl = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    k = [up[i] / kl for i in range(3)]
    th = deg * f * (math.pi / 180.0)
    c, s = math.cos(th), math.sin(th)
    v = [lf[i] - la[i] for i in range(3)]
    kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
    kx = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    frm = [la[i] + v[i] * c + kx[i] * s + k[i] * kv * (1.0 - c) for i in range(3)]
    return host.camera_derive_lens(frm, la, up, cam[9], cam[10], lens[0], lens[1])


@pytest.mark.gpu
def test_cli_renders_a_lens_scene_in_every_mode(pkg, host, torch_cuda, tmp_path):
    from PIL import Image
    torch = torch_cuda
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    W, H, N = 48, 32, 6
    cfg = _cfg(DOF)
    cfg.update(width=W, height=H, samples_per_pixel=N)
    p = tmp_path / "dof.json"
    p.write_text(json.dumps(cfg))
    sc, lens = _lens_scene(host, cfg, W, H, N, depth=cfg["max_depth"])
    gs = pkg.hip.HipScene(sc.ptr, 0)
    gs.set_lens(*lens)
    want = _one_shot(torch, gs)[0]
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    run = lambda *a: subprocess.run([exe, str(p), *a], capture_output=True, text=True, timeout=300, env=env)
    r = run(str(tmp_path / "one.png"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "one.png")), want)
    r = run(str(tmp_path / "passes.png"), "--passes", "3")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "passes.png")), want)
    # the pinhole scene (no keys) through the CLI is another picture; aperture 0 is that picture
    p0 = tmp_path / "zero.json"
    cfg0 = json.loads(json.dumps(cfg))
    cfg0["camera"].update(aperture=0, focus_dist=3)
    p0.write_text(json.dumps(cfg0))
    r0 = subprocess.run([exe, str(p0), str(tmp_path / "zero.png")], capture_output=True, text=True, timeout=300, env=env)
    assert r0.returncode == 0, r0.stderr
    plain, _ = _lens_scene(host, _cfg(COVER), W, H, N, depth=cfg["max_depth"])
    pg = pkg.hip.HipScene(plain.ptr, 0)
    pin = _one_shot(torch, pg)[0]
    pg.close()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "zero.png")), pin) and not np.array_equal(pin, want)
    # --frames 2 --orbit 10: each frame's camera re-derived with the lens
    r = run(str(tmp_path / "anim"), "--frames", "2", "--orbit", "10")
    assert r.returncode == 0, r.stderr
    cam = (C.c_double * 11)()
    host.lib().rt_scene_camera(sc._h, cam)
    lens_keys = _lens_of(host, sc)
    for f in range(2):
        d = _orbit_py(list(cam), lens_keys, 10.0, f, host)
        gs.set_camera(d["origin"], d["lower_left_corner"], d["horizontal"], d["vertical"])
        gs.set_lens(d["u"], d["v"], d["lens_radius"])
        frame = _one_shot(torch, gs)[0]
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"anim_{f:03d}.png")), frame), f
        if f == 0:
            assert np.array_equal(frame, want)
    gs.close()


@pytest.mark.gpu
def test_lens_camera_rays_leave_the_lens_and_meet_the_pinhole_ray_on_the_focus_plane(host, tmp_path):
    """rt_core.h lane_begin_sample<true> on the device, for one pixel and its jitter, checked by geometry alone (no formula
    shared with the restatement): every lens ray starts within r of the camera origin in the plane of u and v, and its
    intersection with the focus plane is the pinhole ray's, within a few ulps"""
    exe = str(tmp_path / "lens_ray_device")
    subprocess.run(["hipcc", *HIPFLAGS, os.path.join(ROOT, "tests", "lens_ray_device.hip"), "-o", exe], check=True, timeout=600)
    lf, la, up, aperture, focus = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.8, 7.5
    d = host.camera_derive_lens(lf, la, up, 20.0, 1.5, aperture, focus)
    W, H, px, py, n = 120, 80, 37, 51, 4096
    cam = d["origin"] + d["lower_left_corner"] + d["horizontal"] + d["vertical"] + d["u"] + d["v"] + [d["lens_radius"]]
    seed = np.array([0x1234_5678_9ABC], np.uint64).view(np.float64)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array(cam, np.float64).tobytes() + seed.tobytes() + np.array([W, H, px, py, n], np.uint32).tobytes())
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=120)
    out = np.fromfile(outp, np.float64).reshape(n, 12)
    lo, ld, po, pd = out[:, 0:3], out[:, 3:6], out[:, 6:9], out[:, 9:12]
    org = np.array(lf)
    w = (org - np.array(la)) / np.linalg.norm(org - np.array(la))
    r = aperture / 2.0
    assert (po == org).all()
    off = lo - org
    assert (np.linalg.norm(off, axis=1) <= r * (1 + 1e-12)).all()
    assert np.abs(off @ w).max() <= 1e-15 * 16
    rad = np.linalg.norm(off, axis=1) / r
    assert rad.max() > 0.99 and np.abs(off.mean(axis=0)).max() < 0.05 * r and (rad < 0.5).mean() > 0.2   # (a disc, not a ring)
    # the focus plane: the points x with (x - (org - f w)) . w = 0
    q = org - focus * w

    def on_plane(o, dd):
        t = ((q - o) @ w) / (dd @ w)
        return o + t[:, None] * dd
    a, b = on_plane(lo, ld), on_plane(po, pd)
    assert np.abs(a - b).max() <= 8 * np.finfo(np.float64).eps * np.abs(b).max(), np.abs(a - b).max()
    # ... and the pinhole ray of every sample differs from the lens ray (the lens moved it)
    assert (np.abs(lo - po).max(axis=1) > 0).mean() > 0.99
