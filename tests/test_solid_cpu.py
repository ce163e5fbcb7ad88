"""Solid textures without a GPU: the schema, csrc/common/rt_solid.h built for the host against the restatement of
tests/solid_mini.py bit for bit (on the point classes of tests/solid_points.py, which tests/test_solid_points_gpu.py puts through the
device) and against properties that need no restatement, and a CPU build of the SOLID lane code
(tests/lanesim, a g++ build) against SolidMini on the frames of the GPU parity test."""
import json
import math
import os

import numpy as np
import pytest

import lane_sim
import solid_mini as SM
import solid_points as SP
from solid_points import MODES, mixed as _points      # (the point table this file always drew: now class `mixed` of tests/solid_points.py)

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


# ------------------------------------------------------------------ the classes of tests/solid_points.py (the device test's tables)
# sha256 of mixed(default_rng(seed), n) as this file drew it before the function moved: the tables of the two tests above
MIXED_SHA256 = {(1616, 100_000): "a24b2baf6490555a6c70e917d7749be9d7910143dd87bdd676ec8635604cb955",
                (1607, 105_000): "b823fd8923660997caf5f10c301eb27fa3f38266668f211adc623bd35bc4acdc",
                (1611, 52_500): "85808833db5195fd118c36f2118fcbdcea3e911795b953d715c133cf12dad32e",
                (1626, 52_500): "a230baeda3219d58db5bd7fb50ad5225b5d3ef26e8f46c81c2fb4fc94e84a1d4",
                (1621, 52_500): "57a3546c3736619c16ebd6b8914e6d2de6cfc412c65492e845d278c208ca09bb",
                (1636, 52_500): "b1a22df66c657147495ce059821f4ef0c854ea2bb9a62a677e2829992f6ffcd0"}


def test_mixed_is_the_table_this_file_always_drew():
    import hashlib
    for (seed, n), want in MIXED_SHA256.items():
        assert hashlib.sha256(_points(np.random.default_rng(seed), n).tobytes()).hexdigest() == want, (seed, n)
    assert {(1600 + 10 * m + o, 105_000 if m == SM.MODE_NOISE else 52_500) for m, o in MODES} | {(1616, 100_000)} == set(MIXED_SHA256)
    assert SP.class_points("mixed").tobytes() == _points(np.random.default_rng(1616), 100_000).tobytes()


def test_class_tables_reach_their_edges():
    """the conditions tests/solid_points.py states for its classes, in numpy on the tables themselves"""
    for cls in SP.CLASSES:
        p = SP.class_points(cls)
        assert len(p) >= 100_000 and p.shape[1] == 3 and not p.flags.writeable, cls
        assert len(SP.subset(cls)) >= 2000 and np.isin(SP.edge_rows(cls), SP.subset(cls)).all(), cls
    # tiny_negative: -2^-k on one axis or on all; t = p - floor(p) is exactly 1.0 from k = 54 on and below 1.0 up to k = 53
    p, k, ax = SP.class_points("tiny_negative"), SP.tiny_k(), SP.tiny_axes()
    assert set(k[:SP.TINY_ROUND].tolist()) == set(range(1, 1075)) and (ax.sum(axis=1) == 3).sum() == len(p) // 4
    assert (p[ax] == np.repeat(-np.ldexp(1.0, -k), ax.sum(axis=1))).all() and (np.floor(p[ax]) == -1.0).all()
    t = (p - np.floor(p))
    one = (t == 1.0) & ax
    assert (one.any(axis=1) == (k >= 54)).all() and (t[ax & (k <= 53)[:, None]] < 1.0).all() and not (t[~ax] >= 1.0).any()
    assert (k >= 54).mean() >= 0.25 and (k <= 52).mean() >= 0.25, ((k >= 54).mean(), (k <= 52).mean())
    # octave_overflow: the first octave whose |p 2^j| reaches 2^31 is j at and one ulp outside 2^(31 - j), and j + 1 one ulp inside it
    p = SP.class_points("octave_overflow")
    j, sign, side, axis = (np.tile(a, SP.OCT_ROUNDS) for a in SP.octave_layout())
    big = np.abs(p).max(axis=1)
    assert (big == np.abs(p[np.arange(len(p)), axis])).all()
    first = np.full(len(p), 99)
    for o in range(17, -1, -1):
        first[big * 2.0 ** o >= SP.TWO31] = np.minimum(first[big * 2.0 ** o >= SP.TWO31], o)
    assert (first[side >= 0] == j[side >= 0]).all() and (first[side < 0] == j[side < 0] + 1).all()
    for octaves in (1, 8, 16):
        for o in range(octaves):
            assert ((first == o) & (side >= 0)).sum() >= 1000 and ((j == o) & (side < 0) & (first == o + 1)).sum() >= 500, (octaves, o)
    # int32_wrap: floors at the ends of the int32 range with the three fractions; i + 1 wraps to 0x80000000 where floor = 2^31 - 1
    p = SP.class_points("int32_wrap")
    f = np.floor(p)
    at = np.isin(f, SP.WRAP_FLOORS)
    assert at.any(axis=1).all() and np.isin((p - f)[at], SP.WRAP_FRACS).all()
    assert {(a, b) for a, b in zip(f[at].tolist(), (p - f)[at].tolist())} == {(a, b) for a in SP.WRAP_FLOORS.tolist() for b in SP.WRAP_FRACS.tolist()}
    inside = (np.abs(p) < SP.TWO31).all(axis=1)
    wraps = inside & ((f.astype(np.int64) + 1) == 2 ** 31).any(axis=1)
    assert wraps.mean() >= 0.10 and (inside & (f == -SP.TWO31).any(axis=1)).mean() >= 0.05, (wraps.mean(), inside.mean())
    # lattice_marble: x, y whole, z whole or -2^-k; the phase's x - floor(x) is 0, just below 1.0, and rounds to 1.0
    p = SP.class_points("lattice_marble")
    z = p[:, 2]
    assert (p[:, :2] == np.rint(p[:, :2])).all() and ((z == np.rint(z)) | ((z < 0.0) & (z >= -2.0 ** -70))).all()
    assert {0.0, 1.0, -1.0, SP.TWO31 - 1.0, 1.0 - SP.TWO31} <= set(z.tolist()) and np.signbit(z[z == 0.0]).any() and not np.signbit(z[z == 0.0]).all()
    x, s = SP.marble_phase(p)
    near = np.isin(z, SP.near_whole_phases())
    assert (s == 0.0).sum() >= 10 and (s == 1.0).sum() >= 1000 and (x[s == 1.0] < 0.0).all()
    assert ((s < 1.0) & (s >= 1.0 - 2.0 ** -20) & near).sum() >= 1000 and ((s > 0.0) & (s <= 2.0 ** -20) & near).sum() >= 1000
    assert (np.abs(x[near] - np.rint(x[near])) <= 4.0 * np.spacing(np.abs(x[near]))).all() and near.sum() >= 10_000
    # checker_planes: the parity flips across the pairs below 2^52; everything at or beyond it is even
    p = SP.class_points("checker_planes")
    m = SP.PLANE_PAIRS
    par = SP.numpy_parity(p)
    flips = par[:m] != par[m:]
    beyond = (np.abs(np.floor(p)) >= SP.TWO52).any(axis=1)
    assert flips.mean() >= 0.45 and flips[106:SP.PLANE_BELOW].all(), flips.mean()
    just_below = (p == np.nextafter(SP.TWO52, 0.0)).any(axis=1)           # (one ulp below +2^52 itself: 2^52 - 1/2, whose parity still counts)
    assert beyond[m + SP.PLANE_BELOW:].all() and (beyond | just_below)[SP.PLANE_BELOW:m].all() and not par[beyond].any() and beyond.mean() >= 0.3
    assert just_below.any() and par[just_below & ~beyond].any()
    mags = np.abs(p[m:]).max(axis=1)
    assert all(((mags >= 2.0 ** e) & (mags < 2.0 ** (e + 4))).sum() >= 100 for e in range(8, 52, 4))


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", [c for c in SP.CLASSES if c != "mixed"])
def test_new_classes_host_build_equals_the_restatement_bit_for_bit(solid_sim, cls):
    """>= 2 000 points of the class, the rows that carry its edge among them: rt_solid_noise_factor in every mode of the class, each set in
    thirds over the three seeds; rt_solid_noise under each seed on a third; the checker parity — host build against tests/solid_mini.py, signs
    of zero included.  lattice_marble: N is exactly 0 on the whole table, which is what makes its phase the one the table test looked at."""
    p = SP.class_points(cls)
    q = p[SP.subset(cls)]
    assert len(q) >= 2000
    same = lambda w, g: w == g and math.copysign(1.0, w) == math.copysign(1.0, g)
    for mode, octaves in SP.class_modes(cls):
        for j, seed in enumerate(SP.SEEDS):
            part = q[j::3]
            got = solid_sim.solid_factor_v(part, mode, octaves, seed)
            for pt, g in zip(part.tolist(), got.tolist()):
                assert same(SM.factor(tuple(pt), mode, octaves, seed), g), (cls, pt, mode, octaves, seed, g)
    for j, seed in enumerate(SP.SEEDS):
        part = q[j::3]
        got = solid_sim.solid_noise_v(part, seed)
        for pt, g in zip(part.tolist(), got.tolist()):
            assert same(SM.noise(tuple(pt), seed), g), (cls, pt, seed, g)
    got = solid_sim.solid_checker_v(q)
    assert got.tolist() == [SM.checker_parity(tuple(pt)) for pt in q.tolist()]
    assert np.array_equal(solid_sim.solid_checker_v(p), SP.numpy_parity(p)), "the table test's parity is the header's"
    if cls == "lattice_marble":
        for seed in SP.SEEDS:
            assert not solid_sim.solid_noise_v(p, seed).any()
            assert not solid_sim.solid_factor_v(p, SM.MODE_TURBULENCE, 16, seed).any()
    if cls == "tiny_negative":          # where t rounds to 1.0 the point takes the far corner's value: still a number in range
        assert np.isfinite(solid_sim.solid_noise_v(p, 0)).all() and np.abs(solid_sim.solid_noise_v(p, 0)).max() <= 1.5


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
