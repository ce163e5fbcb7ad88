"""Solid textures without a GPU: the schema, csrc/common/rt_solid.h built for the host against the restatement of
tests/solid_mini.py bit for bit and against properties that need no restatement, and a CPU build of the SOLID lane code
(tests/lanesim, a g++ build) against SolidMini on the frames of the GPU parity test."""
import json
import math
import os

import numpy as np
import pytest

import lane_sim
import solid_mini as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLID_SCENE = os.path.join(ROOT, "scenes", "cover_solid_1200x800_spp128.json")
CHK = '{"Checker":{"even":[0.25,0.5,0.75],"odd":[0.125,1.0,0.3],"scale":2.5}}'


def _cfg(material, radius="1.0"):
    return ('{"width":8,"height":8,"samples_per_pixel":1,"max_depth":2,"sky":{"texture":""},"camera":{"look_from":{"x":0.0,"y":0.0,"z":5.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":0.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":40.0,"aspect":1.0},"objects":['
            '{"center":{"x":0.0,"y":-100.0,"z":0.0},"radius":99.0,"material":{"Lambertian":{"albedo":[0.5,0.5,0.5]}}},'
            '{"center":{"x":0.0,"y":0.0,"z":0.0},"radius":' + radius + ',"material":' + material + '}]}')


# ------------------------------------------------------------------ schema
def test_schema_defaults_and_the_odd_colour_encoding(host, abi):
    assert (abi.RT_MAT_CHECKER, abi.RT_MAT_NOISE, abi.RT_ABI_VERSION) == (6, 7, 5)
    s = host.Scene.loads(_cfg(CHK, "-2.0")).c.spheres[1]       # (a negative radius is allowed, as for Lambertian)
    assert s.kind == abi.RT_MAT_CHECKER and list(s.albedo) == [0.25, 0.5, 0.75] and s.h_offset == 2.5 and s.radius == -2.0
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    assert s.tex_w == f32(0.125) | (f32(1.0) << 32) and s.tex_h == f32(0.3)
    assert (s.tex_w, s.tex_h) == abi.checker_odd_pack((0.125, 1.0, 0.3))
    assert abi.checker_odd_unpack(s.tex_w, s.tex_h) == (0.125, 1.0, float(np.float32(0.3)))
    n = host.Scene.loads(_cfg('{"Noise":{"albedo":[0.5,0.25,1.0],"scale":4.0}}')).c.spheres[1]
    assert n.kind == abi.RT_MAT_NOISE and list(n.albedo) == [0.5, 0.25, 1.0] and n.h_offset == 4.0
    assert (n.tex_id, n.tex_w, n.tex_h) == (0, 7, 0), "defaults: mode noise, 7 octaves, seed 0"
    for i, mode in enumerate(abi.RT_NOISE_MODES):
        m = host.Scene.loads(_cfg('{"Noise":{"albedo":[0.5,0.25,1.0],"scale":4.0,"mode":"%s","octaves":16,"seed":4294967295}}' % mode)).c.spheres[1]
        assert (m.tex_id, m.tex_w, m.tex_h) == (i, 16, 4294967295)
    assert host.Scene.loads(_cfg('{"Noise":{"albedo":[0.5,0.25,1.0],"scale":4.0,"octaves":1}}')).c.spheres[1].tex_w == 1


def test_schema_round_trips_both_variants(host, abi):
    for mat, want in ((CHK, {"Checker": {"even": [0.25, 0.5, 0.75], "odd": [0.125, 1.0, 0.3], "scale": 2.5}}),
                      ('{"Noise":{"albedo":[0.5,0.25,1.0],"scale":4.0}}', {"Noise": {"albedo": [0.5, 0.25, 1.0], "scale": 4.0, "mode": "noise", "octaves": 7, "seed": 0}}),
                      ('{"Noise":{"seed":9,"mode":"marble","albedo":[0.5,0.25,1.0],"octaves":3,"scale":0.5}}',
                       {"Noise": {"albedo": [0.5, 0.25, 1.0], "scale": 0.5, "mode": "marble", "octaves": 3, "seed": 9}})):
        sc = host.Scene.loads(_cfg(mat))
        text = sc.to_json()
        assert json.loads(text)["objects"][1]["material"] == want
        again = host.Scene.loads(text)
        assert again.to_json() == text
        a, b = sc.c.spheres[1], again.c.spheres[1]
        assert bytes(a) == bytes(b), "the RtSphere record survives the round trip bit for bit"
    # the sequence form of the payload, as for every struct variant
    seq = host.Scene.loads(_cfg('{"Checker":[[0.25,0.5,0.75],[0.125,1.0,0.3],2.5]}'))
    assert seq.to_json() == host.Scene.loads(_cfg(CHK)).to_json()


@pytest.mark.parametrize("material,msg", [
    ('{"Checker":{"even":[0.5,0.5,0.5],"odd":[0.1,0.1,0.1],"scale":0.0}}', "scale"),
    ('{"Checker":{"even":[0.5,0.5,0.5],"odd":[0.1,0.1,0.1],"scale":-1.0}}', "scale"),
    ('{"Checker":{"even":[0.5,0.5,0.5],"odd":[0.1,0.1,0.1],"scale":1e999}}', "scale"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":0.0}}', "scale"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":1e999}}', "scale"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":1.0,"octaves":0}}', "octaves"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":1.0,"octaves":17}}', "octaves"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":1.0,"seed":4294967296}}', "seed"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":1.0,"mode":"wood"}}', "unknown mode `wood`"),
    ('{"Noise":{"albedo":[0.5,0.5,0.5],"scale":1.0,"scale":2.0}}', "duplicate field `scale`"),
    ('{"Checker":{"even":[0.5,0.5,0.5],"odd":[0.1,0.1,0.1],"odd":[0.1,0.1,0.1],"scale":1.0}}', "duplicate field `odd`"),
    ('{"Checker":{"even":[0.5,0.5,0.5],"scale":1.0}}', "missing field `odd`"),
    ('{"Checker":{"odd":[0.5,0.5,0.5],"scale":1.0}}', "missing field `even`"),
    ('{"Noise":{"scale":1.0}}', "missing field `albedo`"),
])
def test_schema_errors_name_the_object(host, material, msg):
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_cfg(material))
    assert "objects[1]" in str(e.value) and msg in str(e.value), str(e.value)


def test_old_scenes_have_no_solid(host, abi):
    for path in ("scenes/cfg2_cover_1200x800_spp128.json", "scenes/cfg1_test_800x600_spp16.json", "scenes/cover_fog_1200x800_spp128.json"):
        sc = host.Scene.load(os.path.join(ROOT, path))
        assert all(sc.c.spheres[i].kind < abi.RT_MAT_CHECKER for i in range(sc.c.n_spheres))
        assert '"Checker"' not in sc.to_json() and '"Noise"' not in sc.to_json()


def test_the_example_scene_is_generated(host, abi):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_solid_scene", os.path.join(ROOT, "scenes", "make_solid_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make() == open(SOLID_SCENE).read()
    sc = host.Scene.load(SOLID_SCENE)
    sp = [sc.c.spheres[i] for i in range(sc.c.n_spheres)]
    assert sp[0].kind == abi.RT_MAT_CHECKER and sp[0].radius == 1000.0
    noise = [s for s in sp if s.kind == abi.RT_MAT_NOISE]
    assert {s.tex_id for s in noise} == {0, 1, 2} and [s.radius for s in noise if s.tex_id == 2] == [1.0]


# ------------------------------------------------------------------ rt_solid.h built for the host
@pytest.fixture(scope="module")
def solid_sim(abi):
    return lane_sim.load(abi)


def _points(rng, n):
    """n points: mostly a few cells around the origin (negative coordinates included), some on lattice planes (t_c = 0), some of every
    magnitude, some around +-2^31 and +-2^52, some non-finite"""
    p = rng.uniform(-40.0, 40.0, (n, 3))
    k = n // 10
    p[:k] = np.round(p[:k]) + rng.uniform(0.0, 1.0, (k, 3)) * (rng.random((k, 3)) < 0.5)                 # whole coordinates
    p[k:2 * k] = rng.standard_normal((k, 3)) * 10.0 ** rng.uniform(-8, 12, (k, 1))                      # every magnitude
    edge = np.array([2.0 ** 31, -2.0 ** 31, np.nextafter(2.0 ** 31, 0.0), -np.nextafter(2.0 ** 31, 0.0), np.nextafter(2.0 ** 31, np.inf),
                     2.0 ** 31 - 0.5, -2.0 ** 31 + 0.5, 2.0 ** 30, 2.0 ** 52, -2.0 ** 52, np.nextafter(2.0 ** 52, 0.0), -np.nextafter(2.0 ** 52, 0.0),
                     2.0 ** 52 - 1.0, 2.0 ** 52 + 2.0, 2.0 ** 53, -2.0 ** 63, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-310, -1e-310, -1.0, 1.0, 0.5])
    m = 2 * k
    sel = rng.integers(0, len(edge), (k, 3))
    p[m:m + k] = np.where(rng.random((k, 3)) < 0.4, edge[sel], p[m:m + k])
    for j, e in enumerate(edge):                        # every edge value on every axis at least once
        for c in range(3):
            p[m + k + 3 * j + c, c] = e
    return p


MODES = [(SM.MODE_NOISE, 7), (SM.MODE_TURBULENCE, 1), (SM.MODE_TURBULENCE, 16), (SM.MODE_MARBLE, 1), (SM.MODE_MARBLE, 16)]


@pytest.mark.parametrize("mode,octaves", MODES)
def test_host_build_equals_the_restatement_bit_for_bit(solid_sim, mode, octaves):
    """>= 10^5 points per mode through rt_solid_noise_factor: 105 000 for noise, 2 x 52 500 for turbulence and for marble (octaves 1 and
    16); each set in thirds over the seeds 0, 2^32 - 1 and one in between"""
    n = 105_000 if mode == SM.MODE_NOISE else 52_500
    rng = np.random.default_rng(1600 + 10 * mode + octaves)
    p = _points(rng, n)
    third = n // 3
    for j, seed in enumerate((0, 0xFFFFFFFF, 0x9E3779B9)):
        q = p[j * third:(j + 1) * third]
        got = solid_sim.solid_factor_v(q, mode, octaves, seed)
        for pt, g in zip(q.tolist(), got.tolist()):
            w = SM.factor(tuple(pt), mode, octaves, seed)
            assert w == g and math.copysign(1.0, w) == math.copysign(1.0, g), (pt, mode, octaves, seed, w, g)
        assert ((got >= 0.0) & (got <= 1.0)).all(), "every factor lies in [0, 1]"


def test_noise_and_checker_equal_the_restatement_bit_for_bit(solid_sim):
    rng = np.random.default_rng(1616)
    p = _points(rng, 100_000)
    for seed in (0, 0xFFFFFFFF):
        got = solid_sim.solid_noise_v(p[:50_000] if seed else p[50_000:], seed)
        for pt, g in zip((p[:50_000] if seed else p[50_000:]).tolist(), got.tolist()):
            w = SM.noise(tuple(pt), seed)
            assert w == g and math.copysign(1.0, w) == math.copysign(1.0, g), (pt, seed, w, g)
    got = solid_sim.solid_checker_v(p)
    want = np.array([SM.checker_parity(tuple(pt)) for pt in p.tolist()], np.int32)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    assert 0.3 < got.mean() < 0.6


def test_noise_properties_without_the_restatement(solid_sim):
    rng = np.random.default_rng(1617)
    # exactly 0 at every lattice point (both signs, the int32 extremes included)
    lat = np.concatenate([rng.integers(-1000, 1000, (20_000, 3)), rng.integers(-2 ** 31 + 1, 2 ** 31 - 1, (20_000, 3)),
                          [[-2 ** 31 + 1, 2 ** 31 - 1, 0], [2 ** 31 - 1] * 3]]).astype(np.float64)
    for seed in (0, 77, 0xFFFFFFFF):
        assert not solid_sim.solid_noise_v(lat, seed).any()
    # outside (-2^31, 2^31), NaN and inf: 0
    out = np.array([[2.0 ** 31, 0.5, 0.5], [0.5, -2.0 ** 31, 0.5], [0.5, 0.5, np.nan], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5]])
    assert not solid_sim.solid_noise_v(out, 5).any()
    # |N| <= 1.5 (the bound rt_solid.h proves), and the values do spread
    p = rng.uniform(-300.0, 300.0, (200_000, 3))
    v = solid_sim.solid_noise_v(p, 12345)
    assert np.abs(v).max() <= 1.5 and v.max() > 0.7 and v.min() < -0.7 and abs(v.mean()) < 0.01
    # continuous across cell faces: 10^4 pairs straddling a face by 1e-13 of a cell
    base = rng.uniform(-50.0, 50.0, (10_000, 3))
    axis = rng.integers(0, 3, 10_000)
    face = np.round(base[np.arange(10_000), axis])
    lo, hi = base.copy(), base.copy()
    lo[np.arange(10_000), axis] = face - 1e-13
    hi[np.arange(10_000), axis] = face + 1e-13
    assert (np.floor(lo) != np.floor(hi)).any(axis=1).all()
    for seed in (0, 0xFFFFFFFF):
        assert np.abs(solid_sim.solid_noise_v(lo, seed) - solid_sim.solid_noise_v(hi, seed)).max() <= 1e-12
    # the seed matters
    assert (solid_sim.solid_noise_v(p[:1000], 1) != solid_sim.solid_noise_v(p[:1000], 2)).mean() > 0.9


def test_checker_parity_flips_across_each_plane_family(solid_sim):
    rng = np.random.default_rng(1618)
    base = np.floor(rng.uniform(-200.0, 200.0, (3000, 3))) + rng.uniform(0.1, 0.9, (3000, 3))
    a = solid_sim.solid_checker_v(base)
    for c in range(3):
        step = base.copy()
        step[:, c] += 1.0
        assert (solid_sim.solid_checker_v(step) == 1 - a).all(), c
        step[:, c] += 1.0
        assert (solid_sim.solid_checker_v(step) == a).all(), c
    # just either side of a plane, negative coordinates included
    for c in range(3):
        lo, hi = base.copy(), base.copy()
        lo[:, c] = np.nextafter(np.floor(base[:, c]), -np.inf)
        hi[:, c] = np.floor(base[:, c])
        assert (solid_sim.solid_checker_v(lo) != solid_sim.solid_checker_v(hi)).all(), c
    # the 2^52 bound: at and beyond it (and for NaN / inf) the colour is `even`; just below it the parity still counts
    big = np.array([[2.0 ** 52, 0.5, 0.5], [0.5, -2.0 ** 52, 1.5], [1.5, 0.5, 2.0 ** 60], [np.nan, 1.5, 0.5], [0.5, np.inf, 0.5], [0.5, 1.5, -np.inf]])
    assert not solid_sim.solid_checker_v(big).any()
    below = np.array([[2.0 ** 52 - 1.0, 0.5, 0.5], [2.0 ** 52 - 2.0, 0.5, 0.5], [-(2.0 ** 52 - 1.0), 0.5, 0.5], [2.0 ** 52 - 0.5, 0.5, 0.5]])
    assert solid_sim.solid_checker_v(below).tolist() == [1, 0, 1, 1]


def test_solid_albedo_reads_the_record_in_the_spheres_frame(abi, host, solid_sim):
    """rt_core.h solid_albedo on rt_tables.h's SphereMat records against solid_mini.solid_colour: the frame is the sphere's (centre far
    from the origin), the odd colour comes back out of its bit patterns, the mode / octaves / seed out of their fields"""
    rng = np.random.default_rng(1619)
    for mat in (CHK, '{"Noise":{"albedo":[0.5,0.25,1.0],"scale":4.0}}', '{"Noise":{"albedo":[0.9,0.8,0.7],"scale":2.5,"mode":"turbulence","octaves":4,"seed":4294967295}}',
                '{"Noise":{"albedo":[0.9,0.8,0.7],"scale":1.5,"mode":"marble","octaves":6,"seed":3}}'):
        sc = host.Scene.loads(_cfg(mat, "2.0"))
        s = sc.c.spheres[1]
        s.center[:] = [13.25, -7.5, 101.125]
        d = rng.standard_normal((2000, 3))
        pts = np.ascontiguousarray(np.array(s.center[:]) + 2.0 * d / np.linalg.norm(d, axis=1)[:, None])
        rc, col = solid_sim.solid_albedo_v(sc.ptr, 1, pts)
        assert rc == 0
        want = np.array([SM.solid_colour(s, tuple(s.center), tuple(p)) for p in pts.tolist()], np.float32)
        assert np.array_equal(col.view(np.uint32), want.view(np.uint32)), mat
        assert len(np.unique(col, axis=0)) > (1 if "Checker" in mat else 100)


def test_tables_count_solids_and_refuse_bad_records(abi, solid_sim):
    """through the C structs (what rt_hip_scene_create* sees)"""
    def world(kind, **kw):
        spheres = (abi.RtSphere * 2)()
        for s in spheres:
            s.radius = 1.0
            s.albedo[:] = [0.5, 0.5, 0.5]
        s = spheres[1]
        s.center[:] = [3.0, 0.0, 0.0]
        s.kind, s.h_offset, s.tex_w, s.tex_h, s.tex_id = kind, 2.0, 7, 0, 0
        for k, v in kw.items():
            setattr(s, k, v)
        sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=4, height=4, samples_per_pixel=1, max_depth=2, sky_mode=1, spheres=spheres, n_spheres=2)
        parts, info, _ = solid_sim.tables(sc)      # info = {n_solids, ...}
        return int(parts is None), info
    for kind in (abi.RT_MAT_CHECKER, abi.RT_MAT_NOISE):
        rc, info = world(kind)
        assert rc == 0 and info[0] == 1
        rc, info = world(kind, radius=-1.0)
        assert rc == 0 and info[0] == 1, "negative radii are allowed"
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert world(kind, h_offset=bad)[0] == 1, (kind, bad)
    assert world(abi.RT_MAT_LAMBERTIAN)[1][0] == 0
    assert world(abi.RT_MAT_CHECKER, tex_w=0xFFFFFFFFFFFFFFFF, tex_h=0xFFFFFFFFFFFFFFFF, tex_id=9)[0] == 0, "a checker's words are colour bits"
    for kw in ({"tex_w": 0}, {"tex_w": 17}, {"tex_h": 1 << 32}, {"tex_id": 3}):
        assert world(abi.RT_MAT_NOISE, **kw)[0] == 1, kw
    assert world(abi.RT_MAT_NOISE, tex_w=16, tex_h=(1 << 32) - 1, tex_id=2)[0] == 0
    assert world(8)[0] == 1


# ------------------------------------------------------------------ the SOLID lane code built for the host
SIM_CASES = [("unlit", "plain", 8), ("unlit", "plain", 50), ("unlit", "moving", 8), ("unlit", "medium", 8), ("lit", "plain", 8), ("lit", "moving", 8),
             ("lit", "medium", 8)]


@pytest.mark.parametrize("world,variant,depth", SIM_CASES)
def test_cpu_build_of_the_lane_code_equals_the_restatement(abi, oracle, host, solid_sim, world, variant, depth):
    """rt_core.h's SOLID lane code built for the host (lane_shade<MEDIUM, true> / scatter's solid arm; tests/lanesim/) against SolidMini on
    the pinhole frames of the GPU parity test (24 x 16 at spp 4): tests/parity.py's bar and the exact segment identity"""
    import test_solid_gpu as G
    from parity import assert_parity, pooled_atol
    sc, c1, lens, spp, _ = G.parity_world(host, world, variant, depth)
    rc, rgb, lin, segs = solid_sim.render(sc.ptr, c1)
    assert rc == 0 and rgb.shape == (16, 24, 3)
    m_rgb, m_lin, m_segs, m_disc = G.mini_frame(oracle, abi, host, world, variant, depth)
    assert_parity(rgb, lin, m_rgb, m_lin, f"{world} {variant}", atol=pooled_atol(spp))
    assert segs == m_segs - m_disc, (segs, m_segs, m_disc)
    # the frame does show its solids: not the frame of the same world with the solids' flat `albedo` colours
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > (100 if world == "unlit" else 20)


@pytest.mark.parametrize("moving", [False, True])
def test_cpu_build_of_the_aov_albedo_equals_the_restatement(abi, oracle, host, solid_sim, moving):
    import test_solid_gpu as G
    sc, c1, _ = G._load(host, G._cfg(G._unlit_objs(moving)), 24, 16, 4, 8, seed=3)
    rc, got = solid_sim.aovs(sc.ptr, 4, c1)
    assert rc == 0 and got.shape == (16, 24, 8)
    want = G._mini(oracle, abi, sc, c1).aovs(4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    assert (got[12:, :, 0] > 0.85).any() and (got[12:, :, 0] < 0.25).any(), "both colours of the ground show as albedo"
