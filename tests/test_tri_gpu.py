"""Triangles and meshes on the GPU, through the C ABI: small frames against the restatement (tests/tri_mini.py) and against the
full scan bit for bit; the device form of the limit (rt_core.h quads_hit: one more scalar load per entry, rt_flat_hit) through
rt_hip_quad_probe against the host build bit for bit on the adversarial tables of tests/tri_rays.py, over mixed lists and over 1024 entries;
two checks that need no restatement (two triangles are their parallelogram; the winding of a triangle); and the plumbing on one scene."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import tri_mini as TM
import tri_sim
from parity import assert_parity, pooled_atol
from quad_rays import N_R, T_MAX, _aimed
from test_medium_gpu import _cfg, _lam, _load, _med, _obj, _one_shot, _pt, _same, _stream
from test_quad_gpu import GLASS, LENS_KEYS, _chk, _floor_objs, _hip_scene, _metal, _noi, _quad, _room_objs
from tri_rays import HYP_QUV, exact_rays, tri_device_class_tables

QUADS, SOLID, MEDIUM, MOTION, LENS, ACCUM, HL = 512, 256, 128, 64, 32, 16, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_SCENE = os.path.join(ROOT, "scenes", "cornell_mesh_600x600_spp128.json")
W, H, SPP = 48, 32, 4
CHUNK = N_R


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ------------------------------------------------------------------ worlds
def _tri(a, b, c, mat):
    return {"triangle": [[float(x) for x in p] for p in (a, b, c)], "material": mat}


def _mesh(vertices, faces, mat):
    return {"mesh": {"vertices": [[float(x) for x in v] for v in vertices], "faces": [list(f) for f in faces]}, "material": mat}


def _flat(q, u, v, shape, mat):
    return {"q": _pt(*q), "u": _pt(*u), "v": _pt(*v), "shape": shape, "material": mat}


TETRA = ([(-2.0, -0.5, 1.8), (-0.6, -0.5, 2.0), (-1.2, -0.5, 3.0), (-1.3, 0.8, 2.3)], [(0, 1, 2), (1, 0, 3), (2, 1, 3), (0, 2, 3)])
OCTA_C, OCTA_R = (-1.1, 0.4, 2.6), 0.8
# outward (counter-clockwise seen from outside): for the octant (sx, sy, sz) the order (x, y, z) is outward iff sx sy sz > 0
OCTA = ([tuple(OCTA_C[k] + (OCTA_R * s if k == ax else 0.0) for k in range(3)) for ax in range(3) for s in (1, -1)],
        [(0 + ix, 2 + iy, 4 + iz) if (1 - 2 * ix) * (1 - 2 * iy) * (1 - 2 * iz) > 0 else (0 + ix, 4 + iz, 2 + iy) for ix in (0, 1) for iy in (0, 1) for iz in (0, 1)])
PYRAMID = ([(-1.3, -1, -1.2), (-0.3, -1, -1.2), (-0.3, -1, -0.2), (-1.3, -1, -0.2), (-0.8, 0.6, -0.7)],
           [(0, 1, 2), (0, 2, 3), (0, 4, 1), (1, 4, 2), (2, 4, 3), (3, 4, 0)])


def _tetra_objs(moving=False):
    return _floor_objs(moving, extra=[_mesh(*TETRA, _lam(0.3, 0.7, 0.4))])


def _room_mesh_objs():
    """test_quad_gpu's closed lit room with a pyramid mesh where its box stood (same place in the file)"""
    objs = _room_objs()
    at = [i for i, o in enumerate(objs) if "box" in o]
    assert len(at) == 1
    objs[at[0]] = _mesh(*PYRAMID, _lam(0.73, 0.73, 0.73))
    return objs


PARITY_CASES = [("tetra", 8), ("tetra", 50), ("room", 8), ("glass", 8), ("metal", 8), ("lens_moving", 8), ("medium", 8), ("solid", 8), ("coincident", 8)]
_MINI_CACHE = {}


def parity_cfg(case):
    if case == "room":
        return _cfg(_room_mesh_objs(), sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0))
    if case == "glass":       # a glass gem, wound outward
        return _cfg(_floor_objs(extra=[_mesh(*OCTA, GLASS)]))
    if case == "metal":       # a mirror triangle
        return _cfg(_floor_objs(extra=[_tri((3.2, -0.5, -3), (3.2, -0.5, 3), (3.2, 3.0, 0), _metal((0.95, 0.95, 0.95), 0.0))]))
    if case == "medium":      # a ball of smoke cut by a triangle
        return _cfg(_tetra_objs() + [_obj((-1.0, 0.6, -2.2), 0.9, _med((0.9, 0.6, 0.3), 2.0)),
                                     _tri((-2.5, -0.5, -2.4), (0.5, -0.5, -2.0), (-1.0, 2.5, -2.2), _lam(0.7, 0.3, 0.3))])
    if case == "solid":       # a Checker and a Noise triangle: the pattern's frame is centred at Q
        return _cfg(_floor_objs(extra=[_tri((-6, -0.45, -6), (6, -0.45, 5), (-6, -0.45, 5), _chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 1.5)),
                                       _tri((-4, -0.5, -3.5), (4, -0.5, -3.5), (0, 4, -3.5), _noi((0.9, 0.8, 0.6), 2.0, "marble", 4, 7))]))
    if case == "coincident":  # triangle / quad / triangle in ONE plane, overlapping: the earlier entry shows
        return _cfg([_obj((0, 0.5, 0), 1.0, _lam(0.8, 0.2, 0.2)),
                     _tri((-3, -0.5, -1), (1, -0.5, -1), (-3, 2.5, -1), _lam(0.9, 0.1, 0.1)),
                     _obj((2.2, 0.3, 0.5), 0.8, _metal((0.8, 0.8, 0.9), 0.05)),
                     _quad((-1, -0.5, -1), (3, 0, 0), (0, 2, 0), _lam(0.1, 0.9, 0.1)),
                     _tri((-2, 0, -1), (3, 0, -1), (3, 3, -1), _lam(0.1, 0.1, 0.9)),
                     _quad((-7, -0.5, -7), (14, 0, 0), (0, 0, 14), _lam(0.6, 0.6, 0.5))])
    return _cfg(_tetra_objs("moving" in case), lens=LENS_KEYS if "lens" in case else None)


def parity_world(host, case, depth):
    """(host scene, center1, lens, quads) of one parity case: 48 x 32 at spp 4"""
    sc, c1, lens = _load(host, parity_cfg(case), W, H, SPP, depth, seed=61 + depth)
    assert (c1 is not None) == ("moving" in case) and (lens is not None) == ("lens" in case)
    return sc, c1, lens, sc.quads()


def _mini(oracle, abi, sc, c1=None, lens=None, quads=None):
    L = oracle.lib(abi)
    return TM.TriMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), c1, lens, quads)


def mini_frame(oracle, abi, host, case, depth):
    """TriMini's frame of a parity case, computed once per session and left unchanged (the CPU and the GPU tests share it)"""
    key = (case, depth)
    if key not in _MINI_CACHE:
        sc, c1, lens, quads = parity_world(host, case, depth)
        m = _mini(oracle, abi, sc, c1, lens, quads)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _MINI_CACHE[key] = (rgb, lin, segs, m.discarded)
    return _MINI_CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case,depth", PARITY_CASES)
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case, depth):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against TriMini; the QUADS kernels run (no new key bit);
    the full scan ("variant" 1) gives the same frame bit for bit"""
    sc, c1, lens, quads = parity_world(host, case, depth)
    gs = _hip_scene(pkg, sc, c1, lens, quads)
    n_tri = sum(q.reserved == abi.RT_QUAD_SHAPE_TRIANGLE for q in quads)
    assert gs.query("quads") == len(quads) and gs.query("triangles") == n_tri > 0
    rgb, lin, st = _one_shot(torch, gs)
    k = gs.query("last_kernel")
    assert k & QUADS and not k & 3 and not k & 8 and k < 1024, k
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


# ------------------------------------------------------------------ the device form through rt_hip_quad_probe
PROBE_CLASSES = ["generic", "edges", "hypotenuse", "den", "t_range"]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _c_flat(abi, quv, shape, kind=0):
    r = abi.RtQuad()
    r.q[:] = [float(x) for x in quv[0:3]]; r.u[:] = [float(x) for x in quv[3:6]]; r.v[:] = [float(x) for x in quv[6:9]]
    r.albedo[:] = [0.7, 0.6, 0.5]
    r.kind, r.fuzz_or_ior, r.reserved = kind, 1.5, shape
    return r


def _probe_scene(pkg, abi, flats):
    """a resident scene of the probe library: one small far-away sphere (id 0) and the flat primitives (ids 1 ..)"""
    spheres = (abi.RtSphere * 1)()
    spheres[0].center[:] = [0.0, 0.0, -60.0]
    spheres[0].radius = 0.5
    spheres[0].albedo[:] = [0.6, 0.5, 0.7]
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=2, max_depth=5, sky_mode=abi.RT_SKY_GRADIENT, spheres=spheres,
                     n_spheres=1, seed=4242)
    sc.cam_origin[:] = [0.0, 0.0, 30.0]; sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]; sc.cam_horizontal[:] = [3.0, 0.0, 0.0]; sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=(abi.RtQuad * len(flats))(*flats))
    gs._keep = (sc, spheres)
    return gs


@functools.lru_cache(maxsize=None)
def _class_table(cls):
    out = []
    for quv, rays, closest in tri_device_class_tables(cls):
        for a in (quv, rays, closest):
            a.setflags(write=False)
        out.append((quv, rays, closest))
    return out


@functools.lru_cache(maxsize=None)
def _class_reference(cls):
    """the host build (rt_flat_hit with lim = 1) on the class's table: hit, t, P, normal, front over all its rays, the entry of every ray"""
    L = tri_sim.load()
    parts, which = [], []
    with np.errstate(all="ignore"):
        for k, (quv, rays, closest) in enumerate(_class_table(cls)):
            st, *res = L.flat_hit_v(quv, 1.0, rays, closest)
            assert st == 0, (cls, k)
            parts.append(res)
            which.append(np.full(len(rays), k, np.int32))
    hit, t, P, nrm, front = (np.concatenate([p[i] for p in parts]) for i in range(5))
    return hit, t, P, nrm, front, np.concatenate(which)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", PROBE_CLASSES)
def test_device_tables_on_the_host_build(cls):
    """the inputs of the device test, without a GPU: >= 10^5 rays, and the host build's triangle decisions straddle (a triangle covers an
    eighth of the square the generic rays are aimed at, so the bar is 2 % .. 95 %; the hypotenuse class is about half and half)"""
    hit = _class_reference(cls)[0]
    total, hits = len(hit), int(hit.sum())
    print(f"{cls}: {hits} of {total} rays hit a triangle (host build)")
    assert total >= 100_000 and 0.02 * total < hits < 0.95 * total
    if cls == "hypotenuse":
        assert 0.25 * total < hits < 0.75 * total


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", PROBE_CLASSES)
def test_device_triangle_code_equals_the_host_build(pkg, abi, torch_cuda, cls):
    """one scene per class — the class's entries as triangles — and each entry's rays with their closest-so-far through
    rt_hip_quad_probe(first_quad = k, n_quads = 1), 1 000 rays per launch; against rt_flat_hit(lim = 1) of the host build: accept decision, t,
    P, hit normal, front_face, bit for bit"""
    from test_quad_rays_gpu import _ProbeOut, _assert_probe_equals, _dev
    table = _class_table(cls)
    hit, t, P, nrm, front, which = _class_reference(cls)
    n = len(hit)
    gs = _probe_scene(pkg, abi, [_c_flat(abi, q, abi.RT_QUAD_SHAPE_TRIANGLE) for q, _, _ in table])
    try:
        assert gs.query("quads") == gs.query("triangles") == len(table)
        assert np.frombuffer(gs.table("quad_lim"), np.float64).tolist() == [1.0] * len(table)
        d_rays = _dev(np.concatenate([r for _, r, _ in table]))
        d_closest = _dev(np.concatenate([c for _, _, c in table]))
        out = _ProbeOut(n)
        stream = torch.cuda.current_stream().cuda_stream
        for off in range(0, n, CHUNK):
            m = min(CHUNK, n - off)
            assert (which[off:off + m] == which[off]).all()
            gs.quad_probe(d_rays.data_ptr() + 48 * off, d_closest.data_ptr() + 8 * off, m, int(which[off]), 1, *out.ptrs(off), stream=stream)
        torch.cuda.synchronize()
        got = out.fetch()
    finally:
        gs.close()
    hits = int((got[0] >= 0).sum())
    print(f"{cls}: {hits} of {n} rays hit (device)")
    want_best = np.where(hit == 1, 1 + which, -1).astype(np.int32)
    _assert_probe_equals(cls, got, want_best, t, P, nrm, front)
    assert hits == int(hit.sum())


def _host_scan(L, quvs, lims, first, rays, closest, id_base):
    """quads_hit restated over the host build's single-entry test: entries in order, every accepted t fed forward as the next closest"""
    n = len(rays)
    best, cl = np.full(n, -1, np.int32), np.array(closest, np.float64)
    t, P, nrm, front = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
    for k, (quv, lim) in enumerate(zip(quvs, lims)):
        st, h, tk, Pk, nk, fk = L.flat_hit_v(quv, lim, rays, cl)
        assert st == 0
        h = h == 1
        best[h], cl[h], t[h], P[h], nrm[h], front[h] = id_base + first + k, tk[h], tk[h], Pk[h], nk[h], fk[h]
    return best, t, P, nrm, front


N_MIX = 40
DUP_OF = [4 * m + (m % 2) for m in range(10)]     # entry N_MIX + m is entry DUP_OF[m] again (five parallelograms, five triangles)


def _shape(k):
    return k % 2                                   # even entries parallelograms, odd entries triangles


@functools.lru_cache(maxsize=None)
def _mixed_inputs():
    table = _class_table("generic")[:N_MIX]
    quvs = [q for q, _, _ in table] + [table[i][0] for i in DUP_OF]
    shapes = [_shape(k) for k in range(N_MIX)] + [_shape(i) for i in DUP_OF]
    rays = np.concatenate([r[:103] for _, r, _ in table])            # 4 120 rays: 64 waves + 24 lanes
    closest = np.concatenate([c[:103] for _, _, c in table])
    rng = np.random.default_rng(2600)
    ab = rng.uniform(0.05, 0.45, (20 * len(DUP_OF), 2))              # inside the triangle too
    dup = np.concatenate([_aimed(rng, quvs[i], 20, ab[20 * m:20 * m + 20]) for m, i in enumerate(DUP_OF)])
    for a in (rays, closest, dup):
        a.setflags(write=False)
    return quvs, shapes, rays, closest, dup


@functools.lru_cache(maxsize=None)
def _mixed_reference(first, count):
    quvs, shapes, rays, closest, _ = _mixed_inputs()
    lims = [TM.LIM[s] for s in shapes]
    return _host_scan(tri_sim.load(), quvs[first:first + count], lims[first:first + count], first, rays, closest, 1)


def test_the_mixed_scan_sees_both_shapes():
    """the inputs of the mixed scan on the host build: both shapes win rays, and reading every entry as a parallelogram (or every limit one
    entry late) would give other ids"""
    quvs, shapes, rays, closest, _ = _mixed_inputs()
    best = _mixed_reference(0, len(quvs))[0]
    won = np.unique(best[best >= 0]) - 1
    assert (np.array(shapes)[won] == 0).sum() > 10 and (np.array(shapes)[won] == 1).sum() > 10
    L = tri_sim.load()
    all_quads = _host_scan(L, quvs, [2.0] * len(quvs), 0, rays, closest, 1)[0]
    shifted = _host_scan(L, quvs, [TM.LIM[s] for s in shapes[1:] + shapes[:1]], 0, rays, closest, 1)[0]
    assert (all_quads != best).sum() > 50 and (shifted != best).sum() > 50


@pytest.mark.gpu
def test_mixed_scan_carries_the_closest_and_each_entrys_limit(pkg, abi, torch_cuda):
    """quads_hit over a list that mixes both shapes (entry k's limit must be entry k's): the whole list and a middle range (13, 21) — the
    range's view starts its limits at the range's first entry — against the host loop; rays into entries listed twice: the first copy wins"""
    from test_quad_rays_gpu import _assert_probe_equals, _probe_scan
    quvs, shapes, rays, closest, dup = _mixed_inputs()
    gs = _probe_scene(pkg, abi, [_c_flat(abi, q, s) for q, s in zip(quvs, shapes)])
    try:
        assert gs.query("triangles") == sum(shapes)
        assert np.frombuffer(gs.table("quad_lim"), np.float64).tolist() == [TM.LIM[s] for s in shapes]
        for first, count in ((0, len(quvs)), (13, 21)):
            got = _probe_scan(gs, rays, closest, first, count)
            want = _mixed_reference(first, count)
            _assert_probe_equals(f"mixed scan ({first}, {count})", got, *want)
            assert (want[0] >= 0).sum() > 0.1 * len(rays)
        free = np.full(len(dup), T_MAX)
        got = _probe_scan(gs, dup, free, 0, len(quvs))
        want = _host_scan(tri_sim.load(), quvs, [TM.LIM[s] for s in shapes], 0, dup, free, 1)
        _assert_probe_equals("entries listed twice", got, *want)
        assert (got[0] >= 0).all() and (got[0] < 1 + N_MIX).all(), "a later copy of an entry never wins"
    finally:
        gs.close()


MANY_TARGETS = (0, 511, 512, 1022, 1023)


@functools.lru_cache(maxsize=None)
def _many_inputs():
    """test_quad_rays_gpu's 1024 entries with alternating shapes, and 4 096 rays aimed inside the triangle half of their targets — the first
    5 x 64 at entries 0, 511, 512, 1022 and 1023"""
    from quad_rays import _quads
    rng = np.random.default_rng(2700)
    quvs = _quads(rng, 1024, "generic")
    aim = np.concatenate([np.repeat(MANY_TARGETS, 64), rng.integers(0, 1024, 4096 - 64 * len(MANY_TARGETS))])
    ab = rng.uniform(0.05, 0.6, (4096, 2))              # (straddles a + b = 1)
    rays = np.concatenate([_aimed(rng, quvs[k], 1, ab[i:i + 1], dist=(0.05, 1.5)) for i, k in enumerate(aim)])
    closest = np.where(rng.random(4096) < 0.5, T_MAX, rng.uniform(0.0, 8.0, 4096))
    for a in (quvs, rays, closest):
        a.setflags(write=False)
    return quvs, rays, closest


@functools.lru_cache(maxsize=None)
def _many_reference():
    quvs, rays, closest = _many_inputs()
    return _host_scan(tri_sim.load(), list(quvs), [TM.LIM[_shape(k)] for k in range(1024)], 0, rays, closest, 1)


def test_the_ends_of_the_1024_entry_table_win():
    best = _many_reference()[0]
    for k in MANY_TARGETS:
        assert (best == 1 + k).sum() >= 8, (k, int((best == 1 + k).sum()))
    ids = np.unique(best[best >= 0]) - 1
    assert (ids % 2 == 0).sum() > 150 and (ids % 2 == 1).sum() > 150


@pytest.mark.gpu
def test_1024_entries_alternating_shapes(pkg, abi, torch_cuda):
    """RT_MAX_QUADS entries, parallelogram / triangle in turn: limit offsets up to 8 KB beside record offsets up to 128 KB through the scalar
    loads of quads_hit; the full-range scan equals the host loop in id and record"""
    from test_quad_rays_gpu import _assert_probe_equals, _probe_scan
    quvs, rays, closest = _many_inputs()
    gs = _probe_scene(pkg, abi, [_c_flat(abi, q, _shape(k)) for k, q in enumerate(quvs)])
    try:
        assert gs.query("quads") == abi.RT_MAX_QUADS == 1024 and gs.query("triangles") == 512
        got = _probe_scan(gs, rays, closest, 0, 1024)
    finally:
        gs.close()
    _assert_probe_equals("1024 entries", got, *_many_reference())


# ------------------------------------------------------------------ exact checks with no restatement
def tiling_cfgs():
    """the floor as one Lambertian parallelogram in the plane y = 0 with power-of-two extents, and as its two triangles (Q, u, v) and
    (Q + u + v, -u, -v): n = (0, -256, 0) for all three, so N, w and D (a zero of either sign: D - dot(N, o) is the same for any o off the
    plane) agree, and t, P and the normal of a hit carry the same bits whichever entry reports it"""
    lam = _lam(0.6, 0.6, 0.5)
    spheres = [_obj((0, 1.0, 0), 1.0, _lam(0.8, 0.2, 0.2)), _obj((2.2, 0.8, 0.5), 0.8, _metal((0.8, 0.8, 0.9), 0.05)), _obj((-1.5, 0.5, 2.0), 0.5, GLASS)]
    one = [_flat((-8, 0, -8), (16, 0, 0), (0, 0, 16), "parallelogram", lam)] + spheres
    two = [_flat((-8, 0, -8), (16, 0, 0), (0, 0, 16), "triangle", lam)] + spheres + [_flat((8, 0, 8), (-16, 0, 0), (0, 0, -16), "triangle", lam)]
    return _cfg(one), _cfg(two)


@pytest.mark.gpu
def test_two_triangles_are_their_parallelogram(pkg, abi, host, torch_cuda):
    """the frame of the one-quad floor and of the two-triangle floor are equal bit for bit in linear radiance and RGB8 (and in segments): no
    ray falls between the triangles or hits both differently.  tests/test_tri_cpu.py confirms the same on the CPU build of the lane code
    first (test_two_triangle_floor_on_the_cpu_build), so this is not an artefact of one device."""
    frames = []
    for cfg in tiling_cfgs():
        sc, c1, lens = _load(host, cfg, W, H, SPP, 8, seed=77)
        gs = _hip_scene(pkg, sc, c1, lens, sc.quads())
        frames.append(_one_shot(torch, gs))
        gs.close()
    _same(frames[0], frames[1], "two triangles vs their parallelogram")
    assert frames[0][2]["segments"] == frames[1][2]["segments"] and frames[0][0].any()


def winding_cfg(swap):
    """Lambertian and Metal triangles, each given as (Q, u, v) or as (Q, v, u): the same point set"""
    f = (lambda q, u, v, m: _flat(q, v, u, "triangle", m)) if swap else (lambda q, u, v, m: _flat(q, u, v, "triangle", m))
    return _cfg([f((-7, -0.5, -7), (28, 0, 0), (0, 0, 28), _lam(0.6, 0.6, 0.5)),
                 _obj((0, 0.5, 0), 1.0, _lam(0.8, 0.2, 0.2)),
                 f((-3.5, -0.5, -2.5), (7, 0, 0.5), (0.3, 3.5, 0), _metal((0.9, 0.7, 0.4), 0.2)),
                 _obj((2.2, 0.3, 0.5), 0.8, _metal((0.8, 0.8, 0.9), 0.05)),
                 f((-2.4, -0.5, 1.5), (1.5, 0, 0.8), (0.6, 1.4, 0.2), _lam(0.2, 0.5, 0.8))])


@pytest.mark.gpu
def test_winding(pkg, abi, host, torch_cuda):
    """(Q, v, u) for (Q, u, v): n, N, D, w and den change sign exactly, t, P and the hit normal keep their bits, alpha and beta change places
    and beta + alpha is alpha + beta (IEEE addition commutes); neither material reads front_face: the same frame bit for bit"""
    frames = []
    for swap in (False, True):
        sc, c1, lens = _load(host, winding_cfg(swap), W, H, SPP, 8, seed=49)
        gs = _hip_scene(pkg, sc, c1, lens, sc.quads())
        assert gs.query("triangles") == 3
        frames.append(_one_shot(torch, gs))
        gs.close()
    _same(frames[0], frames[1], "swapped winding")
    assert frames[0][2]["segments"] == frames[1][2]["segments"]


@pytest.mark.gpu
def test_the_exact_hypotenuse_on_the_device(pkg, abi, torch_cuda):
    """Without the host build: against HYP_QUV a ray's alpha and beta are exact (tests/tri_rays.py).  (j / 64, 1 - j / 64) lies ON the hypotenuse
    and is accepted; one ulp of the sum further out — beta + 2^-50, 0 < alpha < 1 — is rejected; the parallelogram of the same Q, u, v accepts both."""
    from test_quad_rays_gpu import _probe_scan
    a = np.arange(0, 65) / 64.0
    rays = np.concatenate([exact_rays(a, 1.0 - a), exact_rays(a[1:-1], (1.0 - a[1:-1]) + 2.0 ** -50)])
    gs = _probe_scene(pkg, abi, [_c_flat(abi, HYP_QUV, abi.RT_QUAD_SHAPE_TRIANGLE), _c_flat(abi, HYP_QUV, abi.RT_QUAD_SHAPE_PARALLELOGRAM)])
    try:
        tri = _probe_scan(gs, rays, np.full(len(rays), T_MAX), 0, 1)[0]
        par = _probe_scan(gs, rays, np.full(len(rays), T_MAX), 1, 1)[0]
    finally:
        gs.close()
    assert tri[:65].tolist() == [1] * 65 and tri[65:].tolist() == [-1] * 63 and par.tolist() == [2] * len(rays)


# ------------------------------------------------------------------ plumbing
@pytest.mark.gpu
def test_plumbing_on_one_triangle_scene(pkg, abi, host, torch_cuda):
    """passes through rt_hip_accumulate / rt_hip_resolve, a second render, rt_hip_scene_update_spheres against a fresh scene (tables
    included), a group of 2 against one rank, the queries"""
    from test_gpu_parity import _with_env
    sc, c1, lens, quads = parity_world(host, "tetra", 8)
    n_tri = sum(q.reserved for q in quads)
    gs = _hip_scene(pkg, sc, None, None, quads)
    assert gs.query("triangles") == n_tri == 4 and gs.query("quads") == 6
    one = _one_shot(torch, gs)
    assert gs.query("last_kernel") == QUADS
    _same(one, _one_shot(torch, gs), "second render")
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
    assert gs.query("last_kernel") == QUADS | ACCUM
    rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    # moved spheres: the flat primitives and their limits stay
    n = sc.c.n_spheres
    c0 = np.array([list(sc.c.spheres[i].center) for i in range(n)])
    new = c0 + np.array([[0.3, 0.1, -0.2], [-0.1, 0.2, 0.3], [0.2, 0.0, 0.1], [0.0, 0.3, -0.3]])
    lim_before = gs.table("quad_lim")
    assert np.frombuffer(lim_before, np.float64).tolist() == [TM.LIM[int(q.reserved)] for q in quads]
    gs.update_spheres(new, None)
    moved = _one_shot(torch, gs)
    assert gs.query("triangles") == n_tri and gs.table("quad_lim") == lim_before
    for i in range(n):
        sc.c.spheres[i].center[:] = new[i]
    fresh = _hip_scene(pkg, sc, None, None, quads)
    want = _one_shot(torch, fresh)
    _same(moved, want, "updated vs fresh")
    for name in ("geom", "cell_word", "cell_items", "large", "quads", "quad_lim"):
        assert gs.table(name) == fresh.table(name), name
    gs.close(); fresh.close()
    # a group of 2 is one rank
    alone = _hip_scene(pkg, sc, None, None, quads)
    frame, st = alone.render_to_host()
    alone.close()
    for world in (1, 2):
        grp = _with_env({"RT_GPUS_EMULATE": "1"}, lambda: pkg.hip.HipGroup(sc.ptr, world, quads=quads))
        out, gst = grp.render_to_host()
        assert np.array_equal(out, frame) and gst["segments"] == st["segments"], world
        grp.close()


@pytest.mark.gpu
def test_a_scene_of_parallelograms_has_no_limit_table(pkg, abi, host, torch_cuda):
    """no triangle: "triangles" is 0 and "quad_lim" is empty — the loop of DESIGN.md §20 runs as it did"""
    import test_quad_gpu as G
    sc, c1, lens, quads = G.parity_world(host, "floor", 8)
    gs = _hip_scene(pkg, sc, c1, lens, quads)
    assert gs.query("triangles") == 0 and gs.table("quad_lim") == b"" and len(gs.table("quads")) == 128 * len(quads)
    gs.close()


@pytest.mark.gpu
def test_abi_refusals(pkg, abi, host, torch_cuda):
    """RtQuad.reserved above 1 is RT_ERR_INVALID (`quad k: bad shape`); RT_MAX_QUADS counts both shapes"""
    sc, _, _ = _load(host, _cfg([_obj((0, 0, 0), 1.0, _lam(0.5, 0.5, 0.5))]), 8, 8, 1, 2)
    quv = [-1.0, -1.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0, 0.0]
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0, quads=[_c_flat(abi, quv, 1), _c_flat(abi, quv, 2)])
    assert e.value.code == abi.RT_ERR_INVALID and "quad 1: bad shape" in str(e.value)
    mixed = [_c_flat(abi, quv, k % 2) for k in range(abi.RT_MAX_QUADS + 1)]
    ok = pkg.hip.HipScene(sc.ptr, 0, quads=mixed[:-1])
    assert ok.query("quads") == 1024 and ok.query("triangles") == 512
    ok.close()
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(sc.ptr, 0, quads=mixed)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
    for kind, msg in ((abi.RT_MAT_TEXTURE, "Texture"), (abi.RT_MAT_LIGHT, "Light"), (abi.RT_MAT_MEDIUM, "Medium")):
        with pytest.raises(pkg.host.RtError) as e:
            pkg.hip.HipScene(sc.ptr, 0, quads=[_c_flat(abi, quv, 1), _c_flat(abi, quv, 1, kind)])
        assert e.value.code == abi.RT_ERR_INVALID and "quad 1" in str(e.value) and msg in str(e.value)


@pytest.mark.gpu
def test_cli_renders_a_cut_of_the_mesh_example(pkg, host, torch_cuda, tmp_path):
    """the CLI's PNG of scenes/cornell_mesh_600x600_spp128.json at 48 x 32 decodes to the library call's bytes"""
    from PIL import Image
    cfg = json.load(open(MESH_SCENE))
    cfg.update(width=W, height=H, samples_per_pixel=4)
    p = tmp_path / "mesh.json"
    p.write_text(json.dumps(cfg))
    sc, c1, ln = _load(host, cfg)
    gs = _hip_scene(pkg, sc, c1, ln, sc.quads())
    want = _one_shot(torch, gs)[0]
    assert gs.query("last_kernel") & QUADS and gs.query("last_kernel") & HL and gs.query("quads") == 39 and gs.query("triangles") == 34
    gs.close()
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    r = subprocess.run([exe, str(p), str(tmp_path / "mesh.png")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "mesh.png")), want)
    assert want.any()
