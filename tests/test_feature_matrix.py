"""Every MEDIUM, SOLID and QUADS instantiation of the megakernel, and every first-hit kernel, against the restatement.

The sweeps of test_medium_layers.py, test_solid_gpu.py and test_quad_gpu.py launch their 64 + 128 + 64 instantiations and compare each
with itself (accumulated passes with the one-shot frame, the grid walk with the full scan).  Here each of their 128 scenes — a scene
serves a key and that key with ACCUM — is compared with QuadMini (tests/quad_mini.py: shutter time, thin lens, media, solids, lights
with the discarded count, flat primitives; plain Python written from the contract) at tests/parity.py's bar, with the exact segment
identity, and the accumulating instantiation is pinned to the same reference through bit-equality with the one-shot frame.

A small frame can agree with the reference without entering the arm under test, so every scene must show, FROM THE REFERENCE'S OWN
PATHS, that each feature of its key was met: WitnessMini counts the accepted hits on a medium, on a solid, on a flat primitive and on a
moving sphere; a lit cell needs discarded light segments, a lens cell a frame that differs from the pinhole's.  The thresholds are
conditions of the test, not measurements: a scene that misses one is changed, not the threshold.  Unmarked twins check the witnesses
without a GPU (all QUADS scenes; the most featureful LDS and L2 cell of the other two sweeps).

The first-hit kernels (rt_aov, rt_aov_quads, rt_surface, rt_surface_quads: 16 + 16 + 4 + 4) are compared bit for bit on the 32 QUADS
scenes and on the unlit general-map LDS cell of each lens x moving x medium x solid combination.

The 32 QUADS scenes hold parallelograms only, so they reach their 84 kernels through the first loop of quads_hit alone.  Each has a mesh
twin (test_quad_gpu._matrix_cfg with mesh=True: a tetrahedron in front of the box; 11 entries, 4 of them triangles) whose one GPU test
sends the same key, and the key with ACCUM, through the other three routes: the scan with the limit table against TriMini
(tests/tri_mini.py) at the parity bar, the structure of §22 bit for bit the scan, and the structure refit (§24) to a geometry where the
mesh and the box have changed places and back, with the first-hit records of all three against the reference in every bit.  MeshWitness
tallies the reference's flat hits by shape (at least 64 scattered hits on each, a first hit on each); an unmarked test per twin shows on
the host build of the walk (tests/flat_bvh_sim.py) that the structure has an inner root, rejects some camera rays at the root and tests
entries in a leaf for others.

test_all_352_keys_belong_to_one_module restates kernel_key_valid and asserts that the key sets of the six sweeps partition it."""
import json
from collections import namedtuple

import numpy as np
import pytest

import flat_bvh_sim
import medium_mini as MM
import mini_oracle as M
import quad_mini as QM
import solid_mini as SM
import test_flat_bvh_gpu as FB
import test_kernel_matrix as KM
import test_lens as TL
import test_medium_layers as ML
import test_motion as TM
import test_quad_gpu as QG
import test_solid_gpu as SG
import tri_mini as TRI
from parity import assert_parity, pooled_atol
from test_medium_gpu import _load, _one_shot, _same, _stream

LDS, SIMPLE, HL, WIDE, ACCUM, LENS, MOTION, MEDIUM, SOLID, QUADS = (1 << b for b in range(10))
SPP = 2
MODS = {"solid": SG, "medium": ML, "quads": QG, "mesh": QG}
Scene = namedtuple("Scene", "family cell")
SCENES = [Scene(f, c) for f in ("solid", "medium", "quads") for c in MODS[f].SWEEP_CELLS]
# the mesh twin of each QUADS cell (test_quad_gpu._matrix_cfg with mesh=True): the same key through the limit table and the structure
MESH = [Scene("mesh", c) for c in QG.SWEEP_CELLS]
N_MESH_FLATS, N_MESH_TRIS = 11, 4
# the four ways a QUADS kernel reaches its flat primitives, and the scenes whose tests send it that way: the first loop of quads_hit
# (lim == nullptr: test_scene_against_the_restatement, test_first_hit_kernels_against_the_restatement), and the three routes of
# test_mesh_scene_through_every_flat_route
FLAT_ROUTES = {"parallelograms only": [s for s in SCENES if s.family == "quads"], "limit table": MESH, "structure": MESH, "refit structure": MESH}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _id(s):
    return s.family + ":" + MODS[s.family].sweep_name(s.cell).replace(" ", ",")


def _key(s):
    return MODS[s.family].sweep_key(s.cell)


def _size(s):
    """(width, height, hits required per feature): what the reference costs decides the frame — the 5 000-sphere L2 worlds at 9 x 6, the
    484-sphere LDS worlds at 18 x 12, the 12-object QUADS worlds at 36 x 24"""
    if s.family in ("quads", "mesh"):
        return 36, 24, 128
    return (18, 12, 32) if s.cell[2] == "lds" else (9, 6, 8)


def _world(host, s, pinhole=False):
    """(host scene, center1, lens, quads) of a scene at its size"""
    w, h, _ = _size(s)
    if s.family == "mesh":
        return QG.sweep_world(host, s.cell, w, h, pinhole=pinhole, mesh=True)
    out = MODS[s.family].sweep_world(host, s.cell, w, h, pinhole=pinhole)
    return out[0], out[1], out[2], (out[3] if s.family == "quads" else None)


def _atan2(oracle, abi):
    L = oracle.lib(abi)
    return lambda y, x: L.rt_oracle_atan2(y, x)


class WitnessMini(QM.QuadMini):
    """QuadMini, counting what its paths met.  hits: the accepted hits that reach scatter, by the feature of the object hit.  first: the
    first hits of aovs() and surface(), which call hit_world once per camera ray and never scatter."""

    KINDS = ("medium", "solid", "flat", "moving")

    def __init__(self, scene, atan2, center1=None, lens=None, quads=None):
        super().__init__(scene, atan2, center1, lens, quads)
        self.moved = [center1 is not None and tuple(center1[i]) != self.c0[i] for i in range(self.n_spheres)]
        self.hits = dict.fromkeys(self.KINDS, 0)
        self.first = None

    def _tally(self, into, i):
        kind = self.obj[i].kind
        into["medium"] += kind == MM.MEDIUM
        into["solid"] += kind in (SM.CHECKER, SM.NOISE)
        into["flat"] += i >= self.n_spheres
        into["moving"] += i < self.n_spheres and self.moved[i]

    def scatter(self, i, d, p, n, front, node):
        self._tally(self.hits, i)
        return super().scatter(i, d, p, n, front, node)

    def hit_world(self, o, d, node=0):
        hit = super().hit_world(o, d, node)
        if self.first is not None:
            if hit is None:
                self.first["miss"] += 1
            else:
                self._tally(self.first, hit[0])
        return hit

    def first_hits(self, record):
        """record() with the first hits it met: (its result, the tally)"""
        self.first = dict.fromkeys(self.KINDS + ("miss",), 0)
        out = record()
        tally, self.first = self.first, None
        return out, tally


class MeshWitness(WitnessMini, TRI.TriMini):
    """TriMini (tests/tri_mini.py: every entry with its limit) under WitnessMini's counting — WitnessMini.hit_world reaches TriMini.hit_world
    through super() — with the accepted flat hits tallied by shape as well"""
    KINDS = WitnessMini.KINDS + ("triangle", "parallelogram")

    def _tally(self, into, i):
        super()._tally(into, i)
        if i >= self.n_spheres:
            into["triangle" if self.quads[i - self.n_spheres].reserved == TRI.SHAPE_TRIANGLE else "parallelogram"] += 1


assert MeshWitness.__mro__[1:4] == (WitnessMini, TRI.TriMini, QM.QuadMini)


def _mini_class(s, witness=True):
    """the restatement of a scene's family: TriMini where an entry may be a triangle"""
    if s.family == "mesh":
        return MeshWitness if witness else TRI.TriMini
    return WitnessMini if witness else QM.QuadMini


def _pixel(m, x, y):
    """MediumMini.render's pixel (x, y): the mean of the pixel's samples in f32"""
    sc = m.sc
    acc = [M.F(0.0)] * 3
    for s in range(sc.samples_per_pixel):
        o, d = m.begin_sample(x, y, s)
        c = m.ray_color(o, d, sc.max_depth, sc.max_depth, 0, 0)
        acc = [acc[k] + c[k] for k in range(3)]
    scale = M.F(1.0) / M.F(sc.samples_per_pixel)
    return np.array([scale * a for a in acc], np.float32)


def _differs_from_the_pinhole(oracle, abi, host, s, lin):
    """the lens witness: the reference's frame of the same world through a pinhole differs from `lin`, the reference's lens frame.
    One differing pixel shows it, so the pinhole frame is rendered pixel by pixel, from the middle row on, until one differs."""
    sc, c1, lens, quads = _world(host, s, pinhole=True)
    assert lens is None
    pin = _mini_class(s, witness=False)(sc.c, _atan2(oracle, abi), c1, None, quads)
    H, W = lin.shape[:2]
    for y in list(range(H // 2, H)) + list(range(H // 2)):
        for x in range(W):
            if not np.array_equal(_pixel(pin, x, y), lin[y, x]):
                return True
    return False


Ref = namedtuple("Ref", "rgb lin segments discarded hits differs")
_REF = {}


def reference(oracle, abi, host, s):
    """the restatement's frame of a scene with its witnesses, computed once per session and left unchanged"""
    if s not in _REF:
        sc, c1, lens, quads = _world(host, s)
        m = _mini_class(s)(sc.c, _atan2(oracle, abi), c1, lens, quads)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        differs = None
        if lens is not None:
            x, y = sc.c.width // 2, sc.c.height // 2     # (_pixel restates render's pixel: checked where it is used)
            assert np.array_equal(_pixel(_mini_class(s, witness=False)(sc.c, _atan2(oracle, abi), c1, lens, quads), x, y), lin[y, x])
            differs = _differs_from_the_pinhole(oracle, abi, host, s, lin)
        _REF[s] = Ref(rgb, lin, segs, m.discarded, dict(m.hits), differs)
    return _REF[s]


def features(s):
    """the features a scene's key names: {name: present}"""
    k = _key(s)
    return dict(lit=bool(k & HL), lens=bool(k & LENS), moving=bool(k & MOTION), medium=bool(k & MEDIUM), solid=bool(k & SOLID), flat=bool(k & QUADS))


SHAPE_HITS = 64     # a mesh twin: scattered hits required on triangles, and on parallelograms


def check_witnesses(s, ref):
    """every feature of the scene's key was met by the reference's paths; in a mesh twin, both shapes of flat primitive were"""
    f, need, what = features(s), _size(s)[2], _id(s)
    if s.family == "mesh":
        for shape in ("triangle", "parallelogram"):
            assert ref.hits[shape] >= SHAPE_HITS, f"{what}: {ref.hits[shape]} hits on a {shape}, {SHAPE_HITS} required"
        assert ref.hits["triangle"] + ref.hits["parallelogram"] == ref.hits["flat"], what
    for name in ("medium", "solid", "flat", "moving"):
        if f[name]:
            assert ref.hits[name] >= need, f"{what}: {ref.hits[name]} hits on a {name} object, {need} required"
        else:
            assert ref.hits[name] == 0, (what, name, ref.hits[name])
    if f["lit"]:
        assert ref.discarded >= 1, f"{what}: no light ray was traced from a hit on a Light"
    else:
        assert ref.discarded == 0, what
    assert (ref.differs is not None) == f["lens"], what
    if f["lens"]:
        assert ref.differs, f"{what}: the lens frame is the pinhole frame"
    assert (ref.lin != 0).mean() > 0.5, f"{what}: {float((ref.lin != 0).mean()):.2f} of the linear values are non-zero"


def _witness_line(ref):
    h = ref.hits
    shapes = f" (triangles {h['triangle']}, parallelograms {h['parallelogram']})" if "triangle" in h else ""
    return f"hits medium {h['medium']} solid {h['solid']} flat {h['flat']}{shapes} moving {h['moving']}, discarded {ref.discarded}, lens differs {ref.differs}"


# ------------------------------------------------------------------ the 128 frame scenes
@pytest.mark.gpu
@pytest.mark.parametrize("s", SCENES, ids=_id)
def test_scene_against_the_restatement(pkg, abi, oracle, host, torch_cuda, s):
    """the one-shot frame of the scene's key at the parity bar with the exact segment identity; the key with ACCUM — passes [1, 2) then
    [0, 1), resolved — bit for bit the one-shot frame, with the same segments; the reference's witnesses"""
    torch = torch_cuda
    key, what = _key(s), _id(s)
    sc, c1, lens, quads = _world(host, s)
    gs = QG._hip_scene(pkg, sc, c1, lens, quads)
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key, (what, gs.query("last_kernel"), key)
    ref = reference(oracle, abi, host, s)
    print(f"{what} key {key}: max |linear diff| {float(np.abs(lin - ref.lin).max()):.3g}, segments gpu {st['segments']} mini {ref.segments} - {ref.discarded}, "
          + _witness_line(ref))
    check_witnesses(s, ref)
    assert_parity(rgb, lin, ref.rgb, ref.lin, what, atol=pooled_atol(SPP))
    assert st["segments"] == ref.segments - ref.discarded, (what, st["segments"], ref.segments, ref.discarded)
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((1, 2), (0, 1)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
    assert gs.query("last_kernel") == key | ACCUM, (what, gs.query("last_kernel"))
    a_rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    a_lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, a_rgb.data_ptr(), a_lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same((rgb, lin), (a_rgb.cpu().numpy(), a_lin.cpu().numpy()), f"{what}: accumulated vs one-shot")
    assert segs == st["segments"], (what, segs, st["segments"])
    gs.close()


def test_the_scenes_reach_the_256_keys():
    """each scene's test asserts last_kernel == its key, then its key | ACCUM: together they are the MEDIUM, SOLID and QUADS key sets"""
    assert len(SCENES) == 128 and [len(MODS[f].SWEEP_CELLS) for f in ("solid", "medium", "quads")] == [64, 32, 32]
    keys = [_key(s) | a for s in SCENES for a in (0, ACCUM)]
    assert len(set(keys)) == 256 and set(keys) == ML.SWEEP_KEYS | SG.SWEEP_KEYS | QG.SWEEP_KEYS
    assert all(not _key(s) & ACCUM for s in SCENES)
    for route, scenes in FLAT_ROUTES.items():       # every QUADS key through every route to the flat primitives
        assert len(scenes) == 32 and {_key(s) | a for s in scenes for a in (0, ACCUM)} == QG.SWEEP_KEYS, route


# the most featureful cell of the two sphere sweeps, with its tables in LDS and in L2: lit, the general colour map, lens, moving (, medium)
TWINS = [Scene("solid", (True, False, form, True, True, True)) for form in ("lds", "l2")] + [Scene("medium", (True, False, form, True, True)) for form in ("lds", "l2")]


@pytest.mark.parametrize("s", [s for s in SCENES if s.family == "quads"] + TWINS + MESH, ids=_id)
def test_witnesses_on_the_reference(abi, oracle, host, s):
    """the witness conditions need no GPU: they are the reference's"""
    assert s in SCENES + MESH
    ref = reference(oracle, abi, host, s)
    print(f"{_id(s)}: segments {ref.segments} - {ref.discarded}, " + _witness_line(ref))
    check_witnesses(s, ref)


# ------------------------------------------------------------------ the first-hit kernels
FH_SIZE = (18, 12)      # the sphere scenes; the QUADS scenes keep their 36 x 24
FIRST_HIT = [s for s in SCENES if s.family == "quads"] + [Scene("first", (with_lens, moving, medium, solid)) for with_lens in (False, True)
                                                          for moving in (False, True) for medium in (False, True) for solid in (False, True)]


def _fh_id(s):
    if s.family in ("quads", "mesh"):
        return _id(s)
    return "spheres:" + ",".join(f"{n}={v}" for n, v in zip(("lens", "moving", "medium", "solid"), s.cell))


def _fh_features(s):
    if s.family in ("quads", "mesh"):
        return features(s)
    with_lens, moving, medium, solid = s.cell
    return dict(lit=False, lens=with_lens, moving=moving, medium=medium, solid=solid, flat=False)


def _fh_world(host, s):
    """(host scene, center1, lens, quads): a QUADS scene, or the unlit general-map LDS cell of the sphere sweep that owns the combination
    — SOLID's, MEDIUM's where no solid is asked for, and the base cell as the LENS and MOTION sweeps dress it where neither is"""
    if s.family in ("quads", "mesh"):
        return _world(host, s)
    with_lens, moving, medium, solid = s.cell
    w, h = FH_SIZE
    if solid:
        return SG.sweep_world(host, (False, False, "lds", with_lens, moving, medium), w, h)[:3] + (None,)
    if medium:
        return ML.sweep_world(host, (False, False, "lds", with_lens, moving), w, h)[:3] + (None,)
    cfg = json.loads(KM._cell_json(False, False, "lds", width=w, height=h, spp=SPP))
    if moving:
        rng = np.random.default_rng(4 + 2 * with_lens)
        for i, o in enumerate(cfg["objects"]):
            if i % 2 == 0:
                cc, off = o["center"], rng.uniform(-0.3, 0.3, 3)
                o["center1"] = {"x": cc["x"] + off[0], "y": cc["y"] + off[1], "z": cc["z"] + off[2]}
    if with_lens:
        cfg["camera"].update(aperture=0.5, focus_dist=7.0)
    return _load(host, cfg, w, h, SPP, cfg["max_depth"]) + (None,)


FirstRef = namedtuple("FirstRef", "aovs aov_first ids kinds ts surface_first")
_FIRST_REF = {}


def first_reference(oracle, abi, host, s):
    if s not in _FIRST_REF:
        sc, c1, lens, quads = _fh_world(host, s)
        m = _mini_class(s)(sc.c, _atan2(oracle, abi), c1, lens, quads)
        aovs, aov_first = m.first_hits(lambda: m.aovs(SPP))
        (ids, kinds, ts), surface_first = m.first_hits(m.surface)
        for a in (aovs, ids, kinds, ts):
            a.setflags(write=False)
        _FIRST_REF[s] = FirstRef(aovs, aov_first, ids, kinds, ts, surface_first)
    return _FIRST_REF[s]


def check_first_hit_witnesses(s, ref):
    """some camera ray's first hit lies on each feature's kind of object, and some ray misses — in the AOV samples and in the surface rays;
    in a mesh twin some first hit is a triangle and some a parallelogram"""
    f, what = _fh_features(s), _fh_id(s)
    for rays, tally in (("aov", ref.aov_first), ("surface", ref.surface_first)):
        if s.family == "mesh":
            assert tally["triangle"] >= 1 and tally["parallelogram"] >= 1, f"{what}: {rays} first hits on {tally['triangle']} triangles, {tally['parallelogram']} parallelograms"
        for name in ("medium", "solid", "flat", "moving"):
            assert (tally[name] >= 1) if f[name] else (tally[name] == 0), f"{what}: {tally[name]} {rays} first hits on a {name} object"
        assert tally["miss"] >= 1, f"{what}: no {rays} ray misses"
    assert (ref.ids == QM.SURFACE_NONE).sum() == ref.surface_first["miss"]


@pytest.mark.gpu
@pytest.mark.parametrize("s", FIRST_HIT, ids=_fh_id)
def test_first_hit_kernels_against_the_restatement(pkg, abi, oracle, host, torch_cuda, s):
    """render_aovs(2) is QuadMini.aovs(2) bit for bit; render_surface is QuadMini.surface() in id, kind and the bits of t"""
    torch = torch_cuda
    f, what = _fh_features(s), _fh_id(s)
    sc, c1, lens, quads = _fh_world(host, s)
    gs = QG._hip_scene(pkg, sc, c1, lens, quads)
    assert (gs.query("solids") > 0) == f["solid"] and (gs.query("media") > 0) == f["medium"] and (gs.query("motion") > 0) == f["moving"], what
    assert gs.query("lens") == f["lens"] and (gs.query("quads") > 0) == f["flat"], what
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(SPP, aov.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    got = aov.cpu().numpy()
    rec = QG._surface(torch, gs)
    gs.close()
    ref = first_reference(oracle, abi, host, s)
    print(f"{what}: first hits aov {ref.aov_first}, surface {ref.surface_first}")
    check_first_hit_witnesses(s, ref)
    assert np.array_equal(got.view(np.uint32), ref.aovs.view(np.uint32)), (what, float(np.abs(got - ref.aovs).max()))
    assert np.array_equal(rec["id"], ref.ids) and np.array_equal(rec["kind"], ref.kinds), what
    assert np.array_equal(rec["t"].view(np.uint64), ref.ts.view(np.uint64)), what


@pytest.mark.parametrize("s", FIRST_HIT + MESH, ids=_fh_id)
def test_first_hit_witnesses_on_the_reference(abi, oracle, host, s):
    ref = first_reference(oracle, abi, host, s)
    print(f"{_fh_id(s)}: first hits aov {ref.aov_first}, surface {ref.surface_first}")
    check_first_hit_witnesses(s, ref)


def test_the_first_hit_scenes_reach_every_kernel():
    """rt_aov / rt_aov_quads<LENS, MOTION, MEDIUM, SOLID>: 16 each; rt_surface / rt_surface_quads<MOTION, MEDIUM>: 4 each (twice over)"""
    assert len(FIRST_HIT) == 48
    for flat in (False, True):
        combos = {tuple(_fh_features(s)[n] for n in ("lens", "moving", "medium", "solid")) for s in FIRST_HIT if _fh_features(s)["flat"] == flat}
        assert len(combos) == 16, flat
    for route, scenes in FLAT_ROUTES.items():       # rt_aov_quads and rt_surface_quads through every route to the flat primitives
        f = [_fh_features(s) for s in scenes]
        assert all(x["flat"] for x in f), route
        assert len({tuple(x[n] for n in ("lens", "moving", "medium", "solid")) for x in f}) == 16, route
        assert len({(x["moving"], x["medium"]) for x in f}) == 4, route


# ------------------------------------------------------------------ the mesh twins: every QUADS kernel through the limit table and the structure
def _frame_and_passes(torch, gs, key, what):
    """the one-shot frame (rgb, lin, stats) of a scene, with last_kernel the key; and the key with ACCUM — passes [1, 2) then [0, 1), resolved
    — bit for bit that frame, with the same segments"""
    one = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key, (what, gs.query("last_kernel"), key)
    acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((1, 2), (0, 1)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
    assert gs.query("last_kernel") == key | ACCUM, (what, gs.query("last_kernel"))
    a_rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
    a_lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, a_rgb.data_ptr(), a_lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (a_rgb.cpu().numpy(), a_lin.cpu().numpy()), f"{what}: accumulated vs one-shot")
    assert segs == one[2]["segments"], (what, segs, one[2]["segments"])
    return one


def _equal_frames(got, want, what):
    _same(got, want, what)
    assert got[2]["segments"] == want[2]["segments"] > 0, (what, got[2]["segments"], want[2]["segments"])


def _first_hit_records_equal(torch, gs, ref, what):
    """render_aovs(2) is the reference's aovs(2) in every bit; render_surface its surface() in id, kind and the bits of t"""
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(SPP, aov.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    got = aov.cpu().numpy()
    rec = QG._surface(torch, gs)
    assert np.array_equal(got.view(np.uint32), ref.aovs.view(np.uint32)), (what, float(np.abs(got - ref.aovs).max()))
    assert np.array_equal(rec["id"], ref.ids) and np.array_equal(rec["kind"], ref.kinds), what
    assert np.array_equal(rec["t"].view(np.uint64), ref.ts.view(np.uint64)), what


@pytest.mark.gpu
@pytest.mark.parametrize("s", MESH, ids=_id)
def test_mesh_scene_through_every_flat_route(pkg, abi, oracle, host, torch_cuda, s):
    """One QUADS cell's key, and that key with ACCUM, through the three routes to the flat primitives that a scene of parallelograms
    never takes.  A, the scan with the limit table: what test_scene_against_the_restatement asserts, against TriMini.  B, the structure:
    A's frames in every bit, and "variant" 1 too.  C, a refit structure: at G' (the mesh and the box have changed places) the frame of a
    fresh scan scene at G', and back at G A's frames again, both updates refits.  D: the first-hit records of A, B and C's final scene are
    the reference's in every bit."""
    torch = torch_cuda
    key, what = _key(s), _id(s)
    sc, c1, lens, quads = _world(host, s)
    ref, fref = reference(oracle, abi, host, s), first_reference(oracle, abi, host, s)
    check_witnesses(s, ref)
    check_first_hit_witnesses(s, fref)
    # A: the scan with the limit table
    gs = QG._hip_scene(pkg, sc, c1, lens, quads)
    assert gs.query("flat_bvh") == 0 and gs.query("quads") == N_MESH_FLATS and gs.query("triangles") == N_MESH_TRIS, what
    assert len(gs.table("quad_lim")) == 8 * N_MESH_FLATS, what
    A = _frame_and_passes(torch, gs, key, what + ", scan")
    print(f"{what} key {key}: max |linear diff| {float(np.abs(A[1] - ref.lin).max()):.3g}, segments gpu {A[2]['segments']} mini {ref.segments} - {ref.discarded}, "
          + _witness_line(ref) + f"; first hits aov {fref.aov_first}, surface {fref.surface_first}")
    assert_parity(A[0], A[1], ref.rgb, ref.lin, what, atol=pooled_atol(SPP))
    assert A[2]["segments"] == ref.segments - ref.discarded, (what, A[2]["segments"], ref.segments, ref.discarded)
    _first_hit_records_equal(torch, gs, fref, what + ", scan")
    gs.close()
    # B: the structure
    gs = FB._bvh_scene(pkg, sc, c1, lens, quads)
    assert gs.query("flat_bvh") > 1 and gs.query("quads") == N_MESH_FLATS and gs.query("triangles") == N_MESH_TRIS, what
    _equal_frames(_frame_and_passes(torch, gs, key, what + ", structure"), A, what + ": structure vs scan")
    gs.set_option("variant", 1)
    brute = _one_shot(torch, gs)
    gs.set_option("variant", 0)
    assert gs.query("last_kernel") == key, what
    _equal_frames(brute, A, what + ": variant 1 on the structure scene")
    _first_hit_records_equal(torch, gs, fref, what + ", structure")
    # C: the structure refit, away and back
    G, G1 = QG.sweep_mesh_geometries(quads)
    gs.update_flats(G1)
    assert gs.query("flat_refits") == 1, what
    moved = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key, what
    fresh = QG._hip_scene(pkg, sc, c1, lens, QG.with_geometry(quads, G1))
    assert fresh.query("flat_bvh") == 0
    want = _one_shot(torch, fresh)
    assert fresh.query("last_kernel") == key, what
    fresh.close()
    _equal_frames(moved, want, what + ": refit at G' vs a fresh scan scene at G'")
    assert not np.array_equal(moved[1].view(np.uint32), A[1].view(np.uint32)), what + ": the frame at G' is the frame at G"
    gs.update_flats(G)
    _equal_frames(_frame_and_passes(torch, gs, key, what + ", refit back"), A, what + ": refit back to G vs scan")
    assert gs.query("flat_refits") == 2 and gs.query("flat_bvh") > 1, what
    _first_hit_records_equal(torch, gs, fref, what + ", refit back")
    gs.close()


_WALKS = {}


def _walk_witness(abi, host, s):
    """FB.walk_witness of a mesh twin's flat primitives under its pinhole camera's pixel-centre rays, once per (solid, hl, medium): the
    geometry and the camera are one for all cells, the sphere count is not"""
    sc, _, lens, quads = _world(host, s, pinhole=True)
    assert lens is None
    rays = FB.surface_rays(sc.c)
    geometry = (rays.tobytes(), QG.sweep_mesh_geometries(quads)[0].tobytes(), sc.c.n_spheres)
    if geometry not in _WALKS:
        _WALKS[geometry] = FB.walk_witness(flat_bvh_sim.load(abi), quads, rays, sc.c.n_spheres)
    return _WALKS[geometry]


@pytest.mark.parametrize("s", MESH, ids=_id)
def test_the_structure_of_a_mesh_scene_is_walked(abi, host, s):
    """route B is no scan by another name: the structure of the twin's 11 entries has an inner root and no always-visited entry, and of
    the pinhole camera's pixel-centre rays some are rejected at the root, some reach an entry test in a leaf, none takes the fallback"""
    w = _walk_witness(abi, host, s)
    print(f"{_id(s)}: {w}")
    assert w["nodes"] > 1 and w["root_count"] == 0 and w["n_always"] == 0, w
    assert w["at_root"] >= 1 and w["in_leaf"] >= 1 and w["fallback"] == 0, w


# ------------------------------------------------------------------ one accounting of all 352 keys
def kernel_key_valid(key):
    """rt_kernel.hip's kernel_key_valid, restated: wide tables know no LDS staging, media, solids or quads; the QUADS kernels keep their
    tables in L2 and use the general colour map"""
    return 0 <= key < 1024 and not (key & WIDE and key & (LDS | MEDIUM | SOLID | QUADS)) and not (key & QUADS and key & (LDS | SIMPLE))


def test_all_352_keys_belong_to_one_module():
    """the key sets of the six sweeps are pairwise disjoint and their union is exactly the valid keys: a new feature bit fails here until
    a module says that it pins the new instantiations"""
    valid = {k for k in range(-1, 1025) if kernel_key_valid(k)}
    assert len(valid) == 352
    owners = {"test_kernel_matrix": KM.ALL_KEYS, "test_lens": TL.SWEEP_KEYS, "test_motion": TM.SWEEP_KEYS, "test_medium_layers": ML.SWEEP_KEYS,
              "test_solid_gpu": SG.SWEEP_KEYS, "test_quad_gpu": QG.SWEEP_KEYS}
    assert [len(v) for v in owners.values()] == [24, 24, 48, 64, 128, 64]
    names = list(owners)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not owners[a] & owners[b], (a, b, sorted(owners[a] & owners[b]))
    union = set().union(*owners.values())
    assert union == valid, (sorted(valid - union), sorted(union - valid))
    assert (KM.ACCUM, KM.WIDE, KM.HL, KM.SIMPLE, KM.LDS) == (ACCUM, WIDE, HL, SIMPLE, LDS)
    assert (QG.QUADS, QG.SOLID, QG.MEDIUM, QG.MOTION, QG.LENS) == (QUADS, SOLID, MEDIUM, MOTION, LENS)
