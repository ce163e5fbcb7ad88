"""Motion blur: a sphere's "center1", rt_scene_motion, the swept-box grid of rt_tables.h, rt_hip_scene_create_moving /
rt_hip_group_create_moving and the MOTION instantiations of the megakernel.

The reference for motion frames is MotionMini here: tests/mini_oracle.py's ray_color and Philox with the contract's lines
restated — each sample's shutter time tau = (philox(pixel, s, NODE_TIME, 0).x >> 8) * 2^-24, every sphere at c0 + dv * tau (dv the
host's f64 difference, a zero component -0.0) for hit_world and the texture's (u, v); light rays still aim at the static light
centres.  Colour is compared at the project's parity bar (tests/parity.py); geometry and paths are exact, so unlit segment counts
are equal.  The grid walk over swept boxes is checked on the CPU (tests/lanesim, a g++ build of rt_tables.h + rt_core.h
hit_world_grid) and on the device (rt_hip_render_rays_probe) against a numpy brute force at each ray's tau."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import adversarial_rays as AR
import lane_sim
import mini_oracle as M
from parity import assert_parity, pooled_atol
from test_kernel_matrix import ALL_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")
MOTION_SCENE = os.path.join(ROOT, "scenes", "cover_motion_1200x800_spp128.json")
TEST = os.path.join(ROOT, "scenes", "cfg1_test_800x600_spp16.json")
TEX = os.path.join(ROOT, "scenes", "cfg3_cover_4k_textured.json")
MOTION = 64    # rt_hip_scene_query("last_kernel") bit of the MOTION instantiations
LENS = 32
SWEEP_KEYS = {MOTION | l | k for k in ALL_KEYS for l in (0, LENS)}   # the 48 that test_every_motion_instantiation_is_launched pins
NODE_TIME = 0xFFFFFFFD
TAU_LAST = 1.0 - 2.0 ** -24


def tau_of(pixel, sample, seed):
    """the contract's shutter time of sample `sample` of pixel `pixel`"""
    w = M.philox4x32_10(pixel, sample, NODE_TIME, 0, seed & M.M32, (seed >> 32) & M.M32)
    return float(w[0] >> 8) * 2.0 ** -24


def dv_of(c0, c1):
    """the host's dv: one f64 subtraction per component, a zero component (c1 == c0, or both NaN) stored as -0.0"""
    return tuple(-0.0 if (b == a or (a != a and b != b)) else b - a for a, b in zip(c0, c1))


def centres_at(c0, dv, tau):
    """numpy restatement of c0 + dv * tau (two f64 roundings per component)"""
    return c0 + dv * np.float64(tau)


def _dv_array(c0, c1):
    return np.where((c1 == c0) | (np.isnan(c0) & np.isnan(c1)), -0.0, c1 - c0)


class MotionMini(M.Mini):
    """Mini.render with the shutter time of the contract: hit_world, the texel's (u, v) and render at each sample's tau
    (and, with `lens` = (u, v, r), the thin lens of DESIGN.md §13 for the camera ray)"""

    def __init__(self, scene, atan2, center1, lens=None):
        super().__init__(scene, atan2)
        self.c0 = [tuple(o.center) for o in self.obj]
        self.dv = [dv_of(c0, tuple(c1)) for c0, c1 in zip(self.c0, center1)]
        self.lens = lens
        self.set_tau(0.0)

    def set_tau(self, tau):
        self.tau = tau
        self.ct = [(c[0] + d[0] * tau, c[1] + d[1] * tau, c[2] + d[2] * tau) for c, d in zip(self.c0, self.dv)]

    def hit_world(self, o, d):                   # raytracer.rs:44-59 + sphere.rs:46-78, every sphere at the sample's tau
        closest, best = M.F64_MAX, None
        a = M.len2(d)
        for i, c in enumerate(self.ct):
            r = self.obj[i].radius
            oc = M.sub(o, c)
            half_b = M.dot(oc, d)
            cc = M.len2(oc) - r * r
            disc = (half_b * half_b) - (a * cc)
            if disc >= 0.0:
                sq = math.sqrt(disc)
                for root in (((-half_b) - sq) / a, ((-half_b) + sq) / a):
                    if root < closest and root > 0.001:
                        closest, best = root, i
                        break
        if best is None:
            return None
        c, r = self.ct[best], self.obj[best].radius
        p = M.add(o, M.muls(d, closest))
        normal = M.divs(M.sub(p, c), r)
        front = M.dot(d, normal) < 0.0
        return best, p, (normal if front else M.neg(normal)), front

    def texel(self, o, p):                       # sphere.rs:35-43 + materials.rs:236-254 with the centre at tau
        c = self.ct[next(i for i, x in enumerate(self.obj) if x is o)]
        n = M.unit(M.sub(p, c))
        u = (self.atan2(n[0], n[2]) / (2.0 * math.pi)) + 0.5
        v = n[1] * 0.5 + 0.5
        rot = u + o.h_offset
        if rot > 1.0:
            rot = rot - 1.0
        uu, vv = rot * float(o.tex_w), (1.0 - v) * float(o.tex_h - 1)
        px = self.tex[o.tex_id]
        base = 3 * (M.trunc_usize(math.floor(vv)) * o.tex_w + M.trunc_usize(math.floor(uu)))
        base = min(base, len(px) - 3)
        return tuple(M.F(px[base + k]) / M.F(255.0) for k in range(3))

    def camera_ray(self, x, y):
        sc = self.sc
        W, H = sc.width, sc.height
        org, ll, hor, ver = (tuple(v) for v in (sc.cam_origin, sc.cam_lower_left, sc.cam_horizontal, sc.cam_vertical))
        w = self.words(M.NODE_CAMERA, 0)
        u = (float(x) + M.u01_53(w[0], w[1])) / (float(W) - 1.0)
        v = (float(H) - (float(y) + M.u01_53(w[2], w[3]))) / (float(H) - 1.0)
        d = M.sub(M.add(M.add(ll, M.muls(hor, u)), M.muls(ver, v)), org)
        if self.lens is None:
            return org, d
        lu, lv, r = self.lens
        a = 0
        while True:                               # the lens point: NODE_CAMERA slots 1, 2, ...
            ww = self.words(M.NODE_CAMERA, 1 + a)
            pt = next(((M.range_m1_1(p), M.range_m1_1(q)) for p, q in ((ww[0], ww[1]), (ww[2], ww[3]))
                       if M.range_m1_1(p) ** 2 + M.range_m1_1(q) ** 2 < 1.0), None)
            if pt is not None:
                break
            a += 1
        off = M.add(M.muls(tuple(lu), r * pt[0]), M.muls(tuple(lv), r * pt[1]))
        return M.add(org, off), M.sub(d, off)

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
                    w = self.words(NODE_TIME, 0)
                    self.set_tau(float(w[0] >> 8) * 2.0 ** -24)
                    o, d = self.camera_ray(x, y)
                    c = self.ray_color(o, d, sc.max_depth, sc.max_depth, 0, 0)
                    acc = [acc[k] + c[k] for k in range(3)]
                scale = M.F(1.0) / M.F(spp)
                for k in range(3):
                    lin[y, x, k] = scale * acc[k]
                    g = np.sqrt(scale * acc[k]) * M.F(255.0)
                    rgb[y, x, k] = 255 if g != g else int(np.rint(min(max(g, M.F(0.0)), M.F(255.0))))
        return rgb, lin, self.segments


# ---------------------------------------------------------------------------------------------------- scenes of the tests

def _moving_cfg(path, rng, moves, lens=None, skip_lights=True):
    """a scene config whose spheres selected by moves(i, obj) -> offset or None get center1 = center + offset"""
    with open(path) as f:
        cfg = json.load(f)
    for i, o in enumerate(cfg["objects"]):
        if skip_lights and "Light" in o["material"]:
            continue
        off = moves(i, o, rng)
        if off is not None:
            c = o["center"]
            o["center1"] = {"x": c["x"] + off[0], "y": c["y"] + off[1], "z": c["z"] + off[2]}
    if lens:
        cfg["camera"].update(lens)
    return cfg


def _load(host, cfg, w, h, spp, depth=8, seed=None):
    """(host scene, center1 list or None, lens (u, v, r) or None) with the camera in RtScene (the lens's focus-plane camera if any)"""
    sc = host.Scene.loads(json.dumps(cfg))
    c = sc.c
    c.width, c.height, c.samples_per_pixel, c.max_depth = w, h, spp, depth
    if seed is not None:
        c.seed = seed
    lens = None
    if cfg["camera"].get("aperture"):
        out = (C.c_double * 2)()
        host.lib().rt_scene_lens(sc._h, out)
        cam = cfg["camera"]
        pt = lambda p: (float(p["x"]), float(p["y"]), float(p["z"]))
        d = host.camera_derive_lens(pt(cam["look_from"]), pt(cam["look_at"]), pt(cam["vup"]), float(cam["vfov"]), float(cam["aspect"]),
                                    out[0], out[1])
        for i in range(3):
            c.cam_origin[i], c.cam_lower_left[i], c.cam_horizontal[i], c.cam_vertical[i] = (d["origin"][i], d["lower_left_corner"][i],
                                                                                             d["horizontal"][i], d["vertical"][i])
        lens = (d["u"], d["v"], d["lens_radius"])
    return sc, sc.center1(), lens


def _bounce(i, o, rng):   # the book's bouncing spheres (small Lambertian ones move up)
    return (0.0, float(rng.uniform(0.0, 0.5)), 0.0) if "Lambertian" in o["material"] and o["radius"] == 0.2 else None


def _every_other(i, o, rng):   # half of the spheres move, diagonally, by up to a radius and more
    return tuple(float(x) for x in rng.uniform(-0.6, 0.6, 3)) if i % 2 == 1 else None


def _textured(i, o, rng):   # the textured spheres move sideways
    return (float(rng.uniform(-0.8, 0.8)), 0.0, float(rng.uniform(-0.3, 0.3))) if "Texture" in o["material"] or i % 3 == 0 else None


# ---------------------------------------------------------------------------------------------------- no GPU needed

def _sphere_text(extra, material='{"Lambertian":{"albedo":[0.5,0.5,0.5]}}', center='{"x":1.0,"y":2.0,"z":3.0}'):
    """the headline scene with one more sphere object whose map holds `extra` (raw JSON members)"""
    cfg = json.load(open(COVER))
    text = json.dumps(cfg, separators=(",", ":"))
    assert text.endswith("]}")
    return text[:-2] + ',{"center":' + center + extra + ',"radius":0.5,"material":' + material + "}]}"


def test_schema_defaults_and_round_trip(host):
    plain = host.Scene.load(COVER)
    assert plain.center1() is None                       # no key anywhere: rt_scene_motion is NULL
    assert "center1" not in plain.to_json()
    sc = host.Scene.load(MOTION_SCENE)
    c1 = sc.center1()
    n = sc.c.n_spheres
    assert len(c1) == n == 484
    moving = [i for i in range(n) if list(sc.c.spheres[i].center) != c1[i]]
    assert len(moving) == 405
    for i in range(n):
        o = sc.c.spheres[i]
        if i not in moving:
            assert c1[i] == list(o.center)               # a sphere without the key: center1 = center
        else:
            assert c1[i][0] == o.center[0] and c1[i][2] == o.center[2] and 0.0 <= c1[i][1] - o.center[1] < 0.5
    # the RtScene of a motion file is the static file's, field for field
    for i in range(n):
        assert list(sc.c.spheres[i].center) == list(plain.c.spheres[i].center)
    # to_json writes center1 only for the spheres whose file had it, and round-trips
    text = sc.to_json()
    assert text.count('"center1"') == 405
    again = host.Scene.loads(text)
    assert again.center1() == c1 and again.to_json() == text
    # a key equal to the centre is still written (the file had it) and still static
    s2 = host.Scene.loads(_sphere_text(',"center1":{"x":1.0,"y":2.0,"z":3.0}'))
    assert s2.center1()[-1] == [1.0, 2.0, 3.0] and s2.to_json().count('"center1"') == 1
    # integer literals, key order
    s3 = host.Scene.loads(_sphere_text(',"center1":{"z":4,"y":2,"x":1}'))
    assert s3.center1()[-1] == [1.0, 2.0, 4.0]


def test_sequence_form_stays_three_fields(host, abi):
    cfg = json.load(open(COVER))
    o = cfg["objects"][1]
    cfg["objects"][1] = [o["center"], o["radius"], o["material"]]
    sc = host.Scene.loads(json.dumps(cfg))
    assert sc.center1() is None
    cfg["objects"][1] = [o["center"], o["radius"], o["material"], o["center"]]
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(json.dumps(cfg))
    assert e.value.code == abi.RT_ERR_PARSE and "invalid length 4" in str(e.value)


@pytest.mark.parametrize("extra,material,center,msg", [
    (',"center1":{"x":1,"y":2,"z":3},"center1":{"x":1,"y":2,"z":3}', None, None, "duplicate field `center1`"),
    (',"center1":{"x":-1e308,"y":0,"z":0}', None, '{"x":1e308,"y":0,"z":0}', "center1 - center is not finite"),
    (',"center1":{"x":1,"y":2,"z":3.5}', '{"Light":{}}', None, "a Light sphere cannot move"),
    (',"center1":{"x":1,"y":2,"z":3}', '{"Light":[]}', None, "a Light sphere cannot move"),
    (',"center1":{"x":1e999,"y":0,"z":0}', None, None, "out of range"),
    (',"center1":[1,2]', None, None, "invalid length 2"),
    (',"center1":null', None, None, "expected struct Point3D"),
])
def test_schema_errors(host, abi, extra, material, center, msg):
    kw = {}
    if material:
        kw["material"] = material
    if center:
        kw["center"] = center
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_sphere_text(extra, **kw))
    assert e.value.code == abi.RT_ERR_PARSE and msg in str(e.value), str(e.value)
    if "center1" in msg or "Light" in msg or "not finite" in msg:
        assert "objects[484]" in str(e.value), str(e.value)   # (the message names the sphere)


@pytest.fixture(scope="module")
def motion_walk(abi):
    """tests/lanesim: rt_tables.h's motion tables and rt_core.h's hit_world_grid through MotionTables, g++ build"""
    return lane_sim.load(abi)


def test_dv_table_is_the_contract_bit_for_bit(host, motion_walk):
    sc = host.Scene.load(MOTION_SCENE)
    c0 = np.array([list(sc.c.spheres[i].center) for i in range(sc.c.n_spheres)])
    c1 = np.array(sc.center1())
    rc, tab, info = motion_walk.motion_table(sc.ptr, c1)
    assert rc == 0 and info[0] == 405
    want = _dv_array(c0, c1)
    assert np.array_equal(tab[:, :3].view(np.uint64), want.view(np.uint64))      # (-0.0 where nothing moves: the sign bit too)
    assert np.signbit(tab[:, 0]).all() and np.signbit(tab[:, 2]).all()
    assert np.array_equal(tab[:, 3], (np.abs(want) > 0).any(axis=1).astype(np.float64))
    # +0 / -0 centre components: c0 + (-0.0) * tau gives c0's bits back for every tau of the grid's ends
    for z in (0.0, -0.0, 5e-324, -1.5, 1e300):
        for tau in (0.0, TAU_LAST, 0.5):
            assert np.array_equal(np.float64(z) + np.float64(-0.0) * np.float64(tau), np.float64(z)) and \
                np.signbit(np.float64(z) + np.float64(-0.0) * np.float64(tau)) == np.signbit(np.float64(z))
    # a center1 equal to every centre, or none: the static scene (no table), and the same grid as without motion
    rc0, _, info0 = motion_walk.motion_table(sc.ptr, None)
    rc1, _, info1 = motion_walk.motion_table(sc.ptr, c0)
    assert rc0 == rc1 == 2 and np.array_equal(info0, info1)
    # refused: a moving Light sphere, a non-finite difference
    test = host.Scene.load(TEST)
    lights = test.lights()
    tc = np.array([list(test.c.spheres[i].center) for i in range(test.c.n_spheres)])
    bad = tc.copy(); bad[lights[0], 1] += 1.0
    assert motion_walk.motion_table(test.ptr, bad)[0] == 1
    bad = tc.copy(); bad[0, 0] = np.inf
    assert motion_walk.motion_table(test.ptr, bad)[0] == 1


MOTION_WORLDS = {
    # (adversarial world, motion): along one axis, diagonal, across many cells, far from the origin with small cells (forced grid)
    "axis": (0, "axis", {}),
    "diagonal": (3, "diag", {}),
    "many_cells": (1, "long", {}),
    "layer": (4, "axis", {}),
    "far_small_cells": (3, "diag", {"RT_GRID_N": "48,48,48"}),
    "dense": (2, "long", {}),
}


def _world_motion(rng, spheres, n, kind):
    """center1 (n_total x 3) for the first n spheres of an adversarial world; the rest (the ground) static"""
    tot = len(spheres)
    c0 = np.array([spheres[i].center[:] for i in range(tot)], np.float64)
    c1 = c0.copy()
    for i in range(n):
        if i % 4 == 3:
            continue     # (some spheres stay static among the moving ones)
        if kind == "axis":
            off = np.zeros(3); off[i % 3] = rng.uniform(-1.0, 1.0)
        elif kind == "diag":
            off = rng.uniform(-0.7, 0.7, 3)
        else:
            off = rng.uniform(-1.0, 1.0, 3); off *= rng.uniform(2.0, 8.0) / np.linalg.norm(off)
        c1[i] = c0[i] + off
    return c0, c1


@pytest.mark.parametrize("name", sorted(MOTION_WORLDS))
def test_swept_grid_walk_equals_brute_force(abi, motion_walk, monkeypatch, name):
    """hit_world_grid over the motion tables (CPU build) against a numpy brute force at each ray's tau, on the adversarial ray
    families of tests/adversarial_rays.py aimed at the spheres where they are at that tau; tau = 0, 1 - 2^-24 and random"""
    wi, kind, env = MOTION_WORLDS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(7100 + sorted(MOTION_WORLDS).index(name))
    sc, spheres, n = AR.adversarial_world(abi, rng, wi)
    c0, c1 = _world_motion(rng, spheres, n, kind)
    dv = _dv_array(c0, c1)
    radii = np.array([spheres[i].radius for i in range(len(spheres))], np.float64)
    taus = [0.0, TAU_LAST] + [float(np.float32(rng.integers(0, 1 << 24) * 2.0 ** -24)) for _ in range(6)]
    moved = (abi.RtSphere * len(spheres))()
    C.memmove(moved, spheres, C.sizeof(moved))
    all_rays, all_tau = [], []
    for tau in taus:
        ct = centres_at(c0, dv, tau)
        for i in range(len(spheres)):
            moved[i].center[:] = list(ct[i])
        rays, _ = AR.ray_table(rng, moved, n, 140, list(range(AR.FAMILIES)))
        all_rays.append(rays); all_tau.append(np.full(len(rays), tau, np.float32))
    rays, tau_v = np.concatenate(all_rays), np.concatenate(all_tau)
    c1c = np.ascontiguousarray(c1)
    rc, best, t, work = motion_walk.hit_world_v(sc, rays, c1c, tau=tau_v)
    assert rc == 0
    rc, _, info = motion_walk.motion_table(C.pointer(sc), c1c)
    assert rc == 0 and info[1] > 0, "the world must be gridded"
    k = 0
    for tau, rr in zip(taus, all_rays):
        bb, tb = AR.brute_force_hit_world(rr, centres_at(c0, dv, tau), radii)
        g_b, g_t = best[k:k + len(rr)], t[k:k + len(rr)]
        bad = np.nonzero((g_b != bb) | (g_t.view(np.uint64) != tb.view(np.uint64)))[0]
        assert len(bad) == 0, (name, tau, bad[:5], g_b[bad[:5]], bb[bad[:5]], g_t[bad[:5]], tb[bad[:5]])
        k += len(rr)
    assert (best >= 0).mean() > 0.3       # (the rays do meet the moving spheres)


def test_restatement_with_every_center1_equal_is_mini_bit_for_bit(abi, oracle, host):
    """MotionMini with center1 == center (every dv -0.0) is tests/mini_oracle.py's Mini, bit for bit (lit scene, textures, glass)"""
    for path, w, h in ((TEST, 10, 7), (TEX, 8, 5)):
        sc = host.Scene.load(path)
        c = sc.c
        c.width, c.height, c.samples_per_pixel, c.max_depth = w, h, 2, 6
        L = oracle.lib(abi)
        atan2 = lambda y, x: L.rt_oracle_atan2(y, x)
        want = M.Mini(c, atan2).render()
        got = MotionMini(c, atan2, [list(c.spheres[i].center) for i in range(c.n_spheres)]).render()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and got[2] == want[2]


def test_cover_motion_scene_is_generated_from_the_cover_scene():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_motion_scene", os.path.join(ROOT, "scenes", "make_motion_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make() == open(MOTION_SCENE).read()


# ---------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


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


def _hip_scene(pkg, sc, center1, lens=None, library=None):
    gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=center1)
    if lens:
        gs.set_lens(*lens)
    return gs


def _mini(oracle, abi, sc, center1, lens):
    L = oracle.lib(abi)
    return MotionMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), center1, lens)


MOTION_CASES = {
    # (scene, w, h, spp, depth, motion, lens keys)
    "bouncing_unlit": (COVER, 24, 16, 3, 8, _bounce, None),
    "diagonal_unlit": (COVER, 24, 16, 3, 8, _every_other, None),
    "lit": (TEST, 20, 15, 3, 8, _every_other, None),
    "textured": (TEX, 24, 14, 2, 8, _textured, None),
    "bouncing_lens": (COVER, 24, 16, 3, 8, _bounce, {"aperture": 0.3, "focus_dist": 10.0}),
    "lit_lens": (TEST, 20, 15, 2, 8, _every_other, {"aperture": 0.2, "focus_dist": 2.0}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(MOTION_CASES))
def test_motion_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case):
    torch = torch_cuda
    path, w, h, spp, depth, moves, lens_keys = MOTION_CASES[case]
    rng = np.random.default_rng(500 + sorted(MOTION_CASES).index(case))
    sc, c1, lens = _load(host, _moving_cfg(path, rng, moves, lens_keys), w, h, spp, depth)
    gs = _hip_scene(pkg, sc, c1, lens)
    assert gs.query("motion") > 0
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") & MOTION and bool(gs.query("last_kernel") & LENS) == bool(lens)
    m_rgb, m_lin, m_segs = _mini(oracle, abi, sc, c1, lens).render()
    assert_parity(rgb, lin, m_rgb, m_lin, f"{case} one-shot", atol=pooled_atol(spp))
    if gs.query("n_lights") == 0:
        assert st["segments"] == m_segs, (case, st["segments"], m_segs)
    else:   # the kernel skips exactly the light loops the reference computes and discards (raytracer.rs:124): the C oracle counts them
        o_st = oracle.render(abi, sc.ptr, center1=c1, lens=lens)[2]
        assert o_st["segments"] == m_segs and o_st["segments_discarded"] > 0, (case, o_st["segments"], m_segs, o_st["segments_discarded"])
        assert st["segments"] == o_st["segments"] - o_st["segments_discarded"], (case, st["segments"], o_st["segments"], o_st["segments_discarded"])
    # motion changes the picture: the static frame of the same scene differs
    still = _hip_scene(pkg, sc, None, lens)
    assert not np.array_equal(_one_shot(torch, still)[1], lin)
    gs.close(); still.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lens_keys", [None, {"aperture": 0.3, "focus_dist": 6.0}])
def test_hidden_mover_leaves_the_frame_unchanged(pkg, host, torch_cuda, lens_keys):
    """an unlit scene with one more sphere, last in object order, whose whole sweep stays inside the opaque Lambertian sphere at
    (-4, 1, 0) (r = 1) with a gap > 0.001: no camera or bounce ray reaches it, so the MOTION kernels — with every other sphere
    static, tested on its own bits — must give the frame without it, byte for byte (no oracle involved)"""
    torch = torch_cuda
    cfg = json.load(open(COVER))
    if lens_keys:
        cfg["camera"].update(lens_keys)
    assert cfg["objects"][-2]["center"] == {"x": -4.0, "y": 1.0, "z": 0.0} and "Lambertian" in cfg["objects"][-2]["material"]
    base, _, lens = _load(host, cfg, 48, 32, 6, depth=10)
    cfg2 = json.loads(json.dumps(cfg))
    cfg2["objects"].append({"center": {"x": -4.3, "y": 1.0, "z": 0.1}, "center1": {"x": -3.7, "y": 1.2, "z": -0.1}, "radius": 0.3,
                            "material": {"Metal": {"albedo": [0.9, 0.1, 0.1], "fuzz": 0.0}}})
    # (the sweep's centres lie within 0.38 of (-4, 1, 0): every point of the mover within 0.68 of it, inside r = 1 with room to spare)
    c = np.array([[-4.3, 1.0, 0.1], [-3.7, 1.2, -0.1]])
    assert max(np.linalg.norm(p - np.array([-4.0, 1.0, 0.0])) for p in c) + 0.3 < 1.0 - 0.001
    hid, c1, lens2 = _load(host, cfg2, 48, 32, 6, depth=10)
    a = _hip_scene(pkg, base, None, lens)
    b = _hip_scene(pkg, hid, c1, lens2)
    assert b.query("motion") == 1 and b.query("n_spheres") == a.query("n_spheres") + 1
    want = _one_shot(torch, a)
    got = _one_shot(torch, b)
    assert b.query("last_kernel") & MOTION
    _same(got, want, "hidden mover")
    assert got[2]["segments"] == want[2]["segments"]
    a.close(); b.close()


@pytest.mark.gpu
def test_every_motion_instantiation_is_launched(pkg, abi, oracle, host, torch_cuda, monkeypatch):
    """each (lights, simple colour, table form) cell of tests/test_kernel_matrix.py with moving spheres, pinhole and lens,
    one-shot and accumulating: the 48 MOTION instantiations, each frame at the parity bar against the restatement, the
    accumulated frame the one-shot's"""
    from test_kernel_matrix import ACCUM, CELLS, _cell_id, _cell_json, _key
    torch = torch_cuda
    seen = {}
    for cell in CELLS:
        hl, simple, form = cell
        for with_lens in (False, True):
            name = _cell_id(cell) + ("/lens" if with_lens else "")
            cfg = json.loads(_cell_json(hl, simple, form, width=9, height=6, spp=2))
            rng = np.random.default_rng(len(seen))
            for i, o in enumerate(cfg["objects"]):
                if i % 2 == 0 and "Light" not in o["material"]:
                    cc = o["center"]
                    off = rng.uniform(-0.3, 0.3, 3)
                    o["center1"] = {"x": cc["x"] + off[0], "y": cc["y"] + off[1], "z": cc["z"] + off[2]}
            if with_lens:
                cfg["camera"].update(aperture=0.5, focus_dist=7.0)
            sc, c1, lens = _load(host, cfg, 9, 6, 2, depth=cfg["max_depth"])
            library = None
            if form == "wide":
                monkeypatch.setenv("RT_GRID_WIDE", "1")
                library = pkg.hip.probe_lib()
            gs = _hip_scene(pkg, sc, c1, lens, library=library)
            monkeypatch.delenv("RT_GRID_WIDE", raising=False)
            extra = MOTION | (LENS if with_lens else 0)
            one = _one_shot(torch, gs)
            k = gs.query("last_kernel")
            assert k == extra | _key(*cell), (name, k)
            seen.setdefault(k, name)
            acc = _accumulated(torch, gs, ((1, 2), (0, 1)), 2)
            k = gs.query("last_kernel")
            assert k == extra | ACCUM | _key(*cell), (name, k)
            seen.setdefault(k, name)
            _same(acc, one, f"{name}: accumulated vs one-shot")
            m_rgb, m_lin, m_segs = _mini(oracle, abi, sc, c1, lens).render()
            assert_parity(one[0], one[1], m_rgb, m_lin, name, atol=pooled_atol(2))
            if not hl:
                assert one[2]["segments"] == m_segs == acc[2], (name, one[2]["segments"], m_segs, acc[2])
            gs.close()
    want = SWEEP_KEYS
    assert len(want) == 48 and set(seen) == want, sorted(set(seen) ^ want)


@pytest.mark.gpu
def test_composition_with_motion(pkg, abi, oracle, host, torch_cuda):
    """passes in any split, adaptive tiles, the AOVs (first hit at the sample's tau), the denoised host form and a 3-rank group all
    give the one-shot motion frame"""
    from test_adaptive import _tiles_match_one_shot
    from test_denoise import _aovs
    torch = torch_cuda
    N = 9
    rng = np.random.default_rng(11)
    cfg = _moving_cfg(COVER, rng, _bounce)
    sc, c1, _ = _load(host, cfg, 40, 24, N)
    gs, ref = _hip_scene(pkg, sc, c1), _hip_scene(pkg, sc, c1)
    one = _one_shot(torch, ref)
    got = _accumulated(torch, gs, ((6, 9), (0, 1), (1, 6)), N)
    _same(got, one, "passes [6, 9) + [0, 1) + [1, 6)")
    assert got[2] == one[2]["segments"]
    # adaptive host form
    sc2, c2, _ = _load(host, cfg, 80, 48, 32)
    ad, ad_ref = _hip_scene(pkg, sc2, c2), _hip_scene(pkg, sc2, c2)
    img, n_t, _ = ad.render_adaptive(0.05, 8)
    assert len(np.unique(n_t)) > 1, np.unique(n_t)
    _tiles_match_one_shot(torch, abi, ad_ref, img, n_t, ad.tile_grid(), what="motion adaptive")
    ad.close(); ad_ref.close()
    # AOVs against the restatement's first hit at each sample's tau
    n = 3
    aov = _aovs(torch, gs, n).cpu().numpy()
    m = _mini(oracle, abi, sc, c1, None)
    want = np.zeros_like(aov)
    W, H = sc.c.width, sc.c.height
    for y in range(H):
        for x in range(W):
            acc = [0.0] * 8
            m.pixel = y * W + x
            for s in range(n):
                m.sample = s
                m.set_tau(tau_of(m.pixel, s, sc.c.seed))
                o, d = m.camera_ray(x, y)
                hit = m.hit_world(o, d)
                if hit is None:
                    alb = m.sky_colour(d)
                else:
                    i, p, nrm, front = hit
                    ob = m.obj[i]
                    alb = (1.0, 1.0, 1.0) if ob.kind in (M.GLASS, M.LIGHT) else tuple(np.float32(a) for a in ob.albedo)
                    t = M.dot(M.sub(p, o), d) / M.len2(d)
                    acc[3] += 1.0 / t
                    acc[4] += nrm[0]; acc[5] += nrm[1]; acc[6] += nrm[2]
                    acc[7] += 1.0
                for k in range(3):
                    acc[k] += float(alb[k])
            want[y, x] = [np.float32(a / float(n)) for a in acc]
    for ch in (0, 1, 2, 4, 5, 6, 7):
        assert np.array_equal(aov[..., ch].view(np.uint32), want[..., ch].view(np.uint32)), ch
    assert np.allclose(aov[..., 3], want[..., 3], rtol=1e-12, atol=0)
    # the denoised host form: K passes give the bytes of one
    d1 = _hip_scene(pkg, sc, c1)
    one_d, _ = d1.refine_to_host_denoised(N)
    for c in (4, 2, 3):
        last, _ = gs.refine_to_host_denoised(c)
    assert np.array_equal(last, one_d)
    d1.close(); gs.close(); ref.close()
    # a 3-rank group (one device, emulated ranks) and its overlap view: the single-GPU frame
    os.environ["RT_GPUS_EMULATE"] = "1"
    try:
        grp = pkg.hip.HipGroup(sc.ptr, 3, center1=c1)
    finally:
        del os.environ["RT_GPUS_EMULATE"]
    assert grp.size == 3
    for _ in range(3):
        g_rgb, g_st = grp.render_to_host()
        assert np.array_equal(g_rgb, one[0]) and g_st["segments"] == one[2]["segments"]
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wi,kind", [(0, "axis"), (3, "diag"), (1, "long")])
def test_render_rays_probe_on_a_moving_world(pkg, abi, torch_cuda, wi, kind):
    """the megakernel's own walk (MOTION kernels): sample 0's (t, sphere) of every pixel equals a numpy brute force at that
    sample's tau, restated from its Philox address"""
    torch = torch_cuda
    W, H = 32, 16
    rng = np.random.default_rng(900 + wi)
    sc, spheres, n = AR.adversarial_world(abi, rng, wi)
    c0, c1 = _world_motion(rng, spheres, n, kind)
    dv = _dv_array(c0, c1)
    radii = np.array([spheres[i].radius for i in range(len(spheres))], np.float64)
    sc.width, sc.height, sc.samples_per_pixel, sc.max_depth, sc.seed = W, H, 2, 3, 12345
    taus = np.array([tau_of(p, 0, sc.seed) for p in range(W * H)])
    moved = (abi.RtSphere * len(spheres))()
    C.memmove(moved, spheres, C.sizeof(moved))
    rays = np.zeros((W * H, 6))
    for p in range(W * H):   # (each ray aimed at the spheres where they are at its own tau)
        ct = centres_at(c0, dv, taus[p])
        i = int(rng.integers(n))
        moved[i].center[:] = list(ct[i])
        o, d = AR.adversarial_ray(rng, moved, n, p % AR.FAMILIES)
        moved[i].center[:] = list(c0[i])
        rays[p, :3], rays[p, 3:] = o, d
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), center1=c1.tolist())
    d_rays = torch.from_numpy(rays.reshape(H, W, 6)).to("cuda:0")
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    first_t = torch.full((H, W), float("nan"), dtype=torch.float64, device="cuda:0")
    first_b = torch.full((H, W), -2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gs.render_rays_probe(d_rays.data_ptr(), rgb.data_ptr(), 0, first_t.data_ptr(), first_b.data_ptr())
    assert gs.query("last_kernel") & MOTION
    p_t, p_b = first_t.cpu().numpy().reshape(-1), first_b.cpu().numpy().reshape(-1)
    for p in range(W * H):
        bb, tb = AR.brute_force_hit_world(rays[p:p + 1], centres_at(c0, dv, taus[p]), radii)
        assert p_b[p] == bb[0] and np.float64(p_t[p]).view(np.uint64) == np.float64(tb[0]).view(np.uint64), (p, taus[p], p_b[p], bb[0], p_t[p], tb[0])
    assert (p_b >= 0).mean() > 0.3
    gs.close()


@pytest.mark.gpu
def test_cli_renders_the_bouncing_scene_in_every_mode(pkg, host, torch_cuda, tmp_path):
    from PIL import Image
    torch = torch_cuda
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    W, H, N = 48, 32, 6
    env0 = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    for lens_keys in (None, {"aperture": 0.2, "focus_dist": 10.0}):
        cfg = json.load(open(MOTION_SCENE))
        cfg.update(width=W, height=H, samples_per_pixel=N)
        if lens_keys:
            cfg["camera"].update(lens_keys)
        tag = "lens" if lens_keys else "pin"
        p = tmp_path / f"motion_{tag}.json"
        p.write_text(json.dumps(cfg))
        sc, c1, lens = _load(host, cfg, W, H, N, depth=cfg["max_depth"])
        gs = _hip_scene(pkg, sc, c1, lens)
        want = _one_shot(torch, gs)[0]
        d_want, _ = _hip_scene(pkg, sc, c1, lens).refine_to_host_denoised(N)

        def run(*a, env=env0):
            r = subprocess.run([exe, str(p), *a], capture_output=True, text=True, timeout=300, env=env)
            assert r.returncode == 0, (a, r.stderr)

        def img(name):
            return np.asarray(Image.open(tmp_path / name))
        run(str(tmp_path / f"{tag}_one.png"))
        assert np.array_equal(img(f"{tag}_one.png"), want), tag
        run(str(tmp_path / f"{tag}_passes.png"), "--passes", "3")
        assert np.array_equal(img(f"{tag}_passes.png"), want), tag
        run(str(tmp_path / f"{tag}_den.png"), "--denoise")
        assert np.array_equal(img(f"{tag}_den.png"), d_want), tag
        run(str(tmp_path / f"{tag}_ad.png"), "--adaptive", "0", "--min-spp", "2")   # (threshold 0: every tile to N)
        assert np.array_equal(img(f"{tag}_ad.png"), want), tag
        run(str(tmp_path / f"{tag}_anim"), "--frames", "2", "--orbit", "10")
        assert np.array_equal(img(f"{tag}_anim_000.png"), want), tag
        run(str(tmp_path / f"{tag}_animf"), "--frames", "2", "--orbit", "10", env=dict(env0, RT_ANIM="frames"))
        assert np.array_equal(img(f"{tag}_animf_000.png"), want) and np.array_equal(img(f"{tag}_animf_001.png"), img(f"{tag}_anim_001.png")), tag
        run(str(tmp_path / f"{tag}_g2.png"), env=dict(env0, RT_GPUS="2", RT_GPUS_EMULATE="1", RT_GATHER="peer"))
        assert np.array_equal(img(f"{tag}_g2.png"), want), tag
        # the static scene through the CLI is another picture
        cfg0 = json.loads(json.dumps(cfg))
        for o in cfg0["objects"]:
            o.pop("center1", None)
        p0 = tmp_path / f"static_{tag}.json"
        p0.write_text(json.dumps(cfg0))
        r = subprocess.run([exe, str(p0), str(tmp_path / f"{tag}_static.png")], capture_output=True, text=True, timeout=300, env=env0)
        assert r.returncode == 0 and not np.array_equal(img(f"{tag}_static.png"), want), tag
        gs.close()


@pytest.mark.gpu
def test_coverage_of_a_sweeping_sphere_matches_the_fraction_of_the_shutter(pkg, abi, torch_cuda):
    """physics, independent of both restatements: a sphere of radius 0.5 sweeps from x = -3 to x = 3 across a black sky seen
    from (0, 0, 10); the AOV coverage of a pixel on its path is the fraction of samples whose camera ray meets it, which must be the
    fraction of the shutter during which the pixel's central ray meets the sphere, within a binomial bound (+ the pixel's width)"""
    from test_denoise import _aovs
    torch = torch_cuda
    W, H, n = 256, 3, 400
    A, B = 8.0, 0.02
    spheres = (abi.RtSphere * 1)()
    spheres[0].center[:] = [-3.0, 0.0, 0.0]
    spheres[0].radius = 0.5
    spheres[0].kind = abi.RT_MAT_LAMBERTIAN
    spheres[0].albedo[:] = [0.5, 0.5, 0.5]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=W, height=H, samples_per_pixel=1, max_depth=2, spheres=spheres, n_spheres=1,
                     sky_mode=0, seed=77)
    sc.cam_origin[:] = [0.0, 0.0, 10.0]
    sc.cam_lower_left[:] = [-A / 2.0, -0.75 * B, 0.0]
    sc.cam_horizontal[:] = [A, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, B, 0.0]
    gs = pkg.hip.HipScene(C.pointer(sc), 0, center1=[[3.0, 0.0, 0.0]])
    cov = _aovs(torch, gs, n).cpu().numpy()[1, :, 7]
    gs.close()
    e = np.array([0.0, 0.0, 10.0])
    taus = (np.arange(200000) + 0.5) / 200000.0
    cx = -3.0 + 6.0 * taus
    for x in range(W):
        X = -A / 2.0 + A * (x + 0.5) / (W - 1)
        u = np.array([X, 0.0, 0.0]) - e
        u /= np.linalg.norm(u)
        rel = np.stack([cx, np.zeros_like(cx), np.zeros_like(cx)], 1) - e
        dist = np.linalg.norm(np.cross(rel, u), axis=1)
        p = float(np.mean(dist < 0.5))
        pixel_w = (A / (W - 1)) / 6.0 * 1.5            # (the jitter moves the ray by up to one pixel: that share of the sweep)
        bound = 4.0 * math.sqrt(max(p * (1.0 - p), 1.0 / n) / n) + pixel_w
        assert abs(cov[x] - p) <= bound, (x, cov[x], p, bound)
    assert cov.max() > 0.1 and cov[0] == 0.0 and cov[-1] == 0.0
