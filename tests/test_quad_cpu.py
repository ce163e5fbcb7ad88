"""Quads and boxes without a GPU: the schema, csrc/common/rt_quad.h built for the host against the restatement of
tests/quad_mini.py bit for bit and against properties that need no restatement, the tables rt_tables.h builds, and a CPU build of the
QUADS lane code (tests/lanesim, a g++ build) against QuadMini on the frames of the GPU parity test."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import lane_sim
import quad_mini as QM
from quad_rays import CLASSES, _aimed, _quads, class_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL_SCENE = os.path.join(ROOT, "scenes", "cornell_spheres_600x600_spp128.json")
LAM = '{"Lambertian":{"albedo":[0.5,0.25,0.75]}}'
SPHERE = '{"center":{"x":0.0,"y":1.0,"z":0.0},"radius":0.5,"material":{"Glass":{"index_of_refraction":1.5}}}'
QUAD = '{"q":{"x":-1.0,"y":0.0,"z":-1.0},"u":{"x":2.0,"y":0.0,"z":0.25},"v":{"x":0.0,"y":0.5,"z":2.0},"material":%s}'


def _cfg(*objects):
    return ('{"width":8,"height":8,"samples_per_pixel":1,"max_depth":2,"sky":{"texture":""},"camera":{"look_from":{"x":0.0,"y":1.0,"z":5.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":0.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":40.0,"aspect":1.0},"objects":[' + ",".join(objects) + ']}')


# ------------------------------------------------------------------ schema
def test_schema_quads_boxes_and_their_order(host, abi):
    assert C.sizeof(abi.RtQuad) == 128 and abi.RT_MAX_QUADS == 1024 and abi.RT_ABI_VERSION == 5
    box = '{"box":{"min":[0.5,-1.0,2.0],"max":[1.5,0.25,4.0]},"material":{"Metal":{"albedo":[0.9,0.8,0.7],"fuzz":0.125}}}'
    sphere2 = '{"center":{"x":3.0,"y":1.0,"z":0.0},"radius":-0.25,"material":' + LAM + '}'
    chk = '{"Checker":{"even":[0.25,0.5,0.75],"odd":[0.125,1.0,0.3],"scale":2.5}}'
    sc = host.Scene.loads(_cfg(QUAD % LAM, SPHERE, box, sphere2, QUAD % chk))
    q = sc.quads()
    assert sc.c.n_spheres == 2 and len(q) == 8, "spheres keep their relative order in RtScene.spheres, quads theirs in rt_scene_quads"
    assert sc.c.spheres[0].kind == abi.RT_MAT_GLASS and sc.c.spheres[1].radius == -0.25
    assert (list(q[0].q), list(q[0].u), list(q[0].v)) == ([-1.0, 0.0, -1.0], [2.0, 0.0, 0.25], [0.0, 0.5, 2.0])
    assert q[0].kind == abi.RT_MAT_LAMBERTIAN and list(q[0].albedo) == [0.5, 0.25, 0.75]
    assert q[7].kind == abi.RT_MAT_CHECKER and q[7].h_offset == 2.5 and (q[7].tex_w, q[7].tex_h) == abi.checker_odd_pack((0.125, 1.0, 0.3))
    # the box: six quads in place, in the header's order, built with its operations
    want = QM.box_quads((0.5, -1.0, 2.0), (1.5, 0.25, 4.0))
    for k in range(6):
        b = q[1 + k]
        assert (tuple(b.q), tuple(b.u), tuple(b.v)) == want[k], k
        assert all(math.copysign(1.0, x) == math.copysign(1.0, y) for got, w in zip((b.q, b.u, b.v), want[k]) for x, y in zip(got, w)), "the zeros are +0.0"
        assert b.kind == abi.RT_MAT_METAL and b.fuzz_or_ior == 0.125
    assert [tuple(b.q) for b in q[1:7]] == [(0.5, -1.0, 4.0), (1.5, -1.0, 4.0), (1.5, -1.0, 2.0), (0.5, -1.0, 2.0), (0.5, 0.25, 4.0), (0.5, -1.0, 2.0)]
    # the box sugar equals its six explicit quads
    pt = lambda p: '{"x":%r,"y":%r,"z":%r}' % p
    explicit = ['{"q":%s,"u":%s,"v":%s,"material":{"Metal":{"albedo":[0.9,0.8,0.7],"fuzz":0.125}}}' % (pt(a), pt(b), pt(c)) for a, b, c in want]
    sc2 = host.Scene.loads(_cfg(QUAD % LAM, SPHERE, *explicit, sphere2, QUAD % chk))
    assert bytes(sc2.quads()) == bytes(q) and sc2.to_json() == sc.to_json()
    # rt_scene_to_json writes the six quads (not the box), in the file's interleaving, and round-trips every RtQuad bit for bit
    text = sc.to_json()
    objs = json.loads(text)["objects"]
    assert ["q" in o for o in objs] == [True, False] + [True] * 6 + [False, True] and not any("box" in o for o in objs)
    again = host.Scene.loads(text)
    assert again.to_json() == text and bytes(again.quads()) == bytes(q)
    assert [bytes(again.c.spheres[i]) for i in range(2)] == [bytes(sc.c.spheres[i]) for i in range(2)]
    # the sequence form of a point, and awkward numbers, survive too
    odd = host.Scene.loads(_cfg('{"q":[0.1,-0.0,1e-300],"u":[3.0000000000000004,0.0,0.0],"v":[0.0,1e150,0.7],"material":' + LAM + '}'))
    back = host.Scene.loads(odd.to_json())
    assert bytes(back.quads()) == bytes(odd.quads()) and math.copysign(1.0, back.quads()[0].q[1]) == -1.0
    # a file without a quad has none, and loads as it always did
    plain = host.Scene.loads(_cfg(SPHERE))
    assert plain.quads() is None and '"q"' not in plain.to_json()
    n = C.c_uint32(7)
    assert not host.lib().rt_scene_quads(plain._h, C.byref(n)) and n.value == 0


@pytest.mark.parametrize("obj,msg", [
    ('{"q":{"x":0,"y":0,"z":0},"center":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":' + LAM + '}', "mixed keys"),
    ('{"q":{"x":0,"y":0,"z":0},"radius":1.0,"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":' + LAM + '}', "mixed keys"),
    ('{"box":{"min":[0,0,0],"max":[1,1,1]},"q":{"x":0,"y":0,"z":0},"material":' + LAM + '}', "mixed keys"),
    ('{"box":{"min":[0,0,0],"max":[1,1,1]},"center":{"x":0,"y":0,"z":0},"material":' + LAM + '}', "mixed keys"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":' + LAM + '}', "duplicate field `u`"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":' + LAM + ',"material":' + LAM + '}', "duplicate field `material`"),
    ('{"box":{"min":[0,0,0],"max":[1,1,1],"min":[0,0,0]},"material":' + LAM + '}', "duplicate field `min`"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"material":' + LAM + '}', "missing field `v`"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0}}', "missing field `material`"),
    ('{"box":{"min":[0,0,0]},"material":' + LAM + '}', "missing field `max`"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"center1":{"x":0,"y":1,"z":0},"material":' + LAM + '}', "center1"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":2,"y":0,"z":0},"material":' + LAM + '}', "degenerate"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":0,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":' + LAM + '}', "degenerate"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1e-170,"y":0,"z":0},"v":{"x":0,"y":1e-170,"z":0},"material":' + LAM + '}', "degenerate"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1e170,"y":0,"z":0},"v":{"x":0,"y":1e170,"z":0},"material":' + LAM + '}', "degenerate"),
    ('{"box":{"min":[0,0,0],"max":[1,0,1]},"material":' + LAM + '}', "min must be below max"),
    ('{"box":{"min":[0,0,2],"max":[1,1,1]},"material":' + LAM + '}', "min must be below max"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":{"Light":{}}}', "cannot be a Light"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":{"Medium":{"albedo":[0.5,0.5,0.5],"density":1.0}}}', "cannot be a Medium"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":{"Texture":{"albedo":[1,1,1],"pixels":"scenes/data/earth.jpg","width":8,"height":8,"h_offset":0.0}}}', "cannot be a Texture"),
    ('{"box":{"min":[0,0,0],"max":[1,1,1]},"material":{"Light":{}}}', "cannot be a Light"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":{"Checker":{"even":[1,1,1],"odd":[0,0,0],"scale":0.0}}}', "scale"),
    ('{"q":{"x":0,"y":0,"z":0},"u":{"x":1,"y":0,"z":0},"v":{"x":0,"y":1,"z":0},"material":{"Noise":{"albedo":[1,1,1],"scale":1.0,"octaves":17}}}', "octaves"),
])
def test_schema_errors_name_the_object_by_the_files_index(host, obj, msg):
    """the bad object is objects[2] of the file — behind a quad and a sphere, so neither the sphere count nor the quad count names it"""
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_cfg(QUAD % LAM, SPHERE, obj))
    assert "objects[2]" in str(e.value) and msg in str(e.value), str(e.value)


def test_sphere_errors_behind_a_quad_keep_the_files_index(host):
    for obj, msg in (('{"center":{"x":0,"y":0,"z":0},"radius":1.0,"center1":{"x":0,"y":1,"z":0},"material":{"Light":{}}}', "cannot move"),
                     ('{"center":{"x":0,"y":0,"z":0},"radius":-1.0,"material":{"Medium":{"albedo":[0.5,0.5,0.5],"density":1.0}}}', "radius"),
                     ('{"center":{"x":0,"y":0,"z":0},"radius":1.0,"material":{"Noise":{"albedo":[1,1,1],"scale":-1.0}}}', "scale")):
        with pytest.raises(host.RtError) as e:
            host.Scene.loads(_cfg(QUAD % LAM, QUAD % LAM, obj))
        assert "objects[2]" in str(e.value) and msg in str(e.value), str(e.value)


def test_the_example_scene_is_generated(host, abi):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cornell_scene", os.path.join(ROOT, "scenes", "make_cornell_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make() == open(CORNELL_SCENE).read()
    sc = host.Scene.load(CORNELL_SCENE)
    q = sc.quads()
    assert len(q) == 17 and all(x.kind == abi.RT_MAT_LAMBERTIAN for x in q) and sc.c.sky_mode == abi.RT_SKY_NONE and sc.c.max_depth == 50
    kinds = sorted(sc.c.spheres[i].kind for i in range(sc.c.n_spheres))
    assert kinds == [abi.RT_MAT_METAL, abi.RT_MAT_GLASS, abi.RT_MAT_LIGHT]
    assert (sc.c.width, sc.c.height, sc.c.samples_per_pixel) == (600, 600, 128)


def test_old_scenes_have_no_quad(host):
    for path in ("scenes/cfg2_cover_1200x800_spp128.json", "scenes/cfg1_test_800x600_spp16.json", "scenes/cover_solid_1200x800_spp128.json"):
        assert host.Scene.load(os.path.join(ROOT, path)).quads() is None


# ------------------------------------------------------------------ rt_quad.h built for the host
@pytest.fixture(scope="module")
def quad_sim(abi):
    return lane_sim.load(abi)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _compare(L, quv, rays, closest, what):
    """the host build against quad_mini on every ray: accept decision, t, P, normal and front_face bit for bit; returns the hit count"""
    st, hit, t, P, nrm, front = L.quad_hit_v(quv, rays, closest)
    c = QM.QuadConsts(quv[0:3], quv[3:6], quv[6:9])
    assert (st == 0) == c.ok, (what, quv)
    if not c.ok:
        return 0
    n_hit = 0
    tb, Pb, nb = _bits(t), _bits(P), _bits(nrm)
    for i, (ray, cl) in enumerate(zip(rays.tolist(), closest.tolist())):
        r = QM.quad_test(c, ray[0:3], ray[3:6], cl)
        if r is None:
            assert not hit[i], (what, quv, ray, cl)
            continue
        n_hit += 1
        f, nm = QM.quad_record(c, ray[3:6])
        assert hit[i] and bool(front[i]) == f, (what, quv, ray, cl)
        assert tb[i] == _bits([r[0]])[0] and Pb[i].tolist() == _bits(r[1]).tolist() and nb[i].tolist() == _bits(nm).tolist(), (what, quv, ray, cl)
    return n_hit


@pytest.mark.filterwarnings("ignore::RuntimeWarning")     # (the classes make NaN, inf and overflow on purpose)
@pytest.mark.parametrize("cls", CLASSES)
def test_host_build_equals_the_restatement_bit_for_bit(quad_sim, cls):
    """>= 10^5 rays per class (tests/quad_rays.py: 100 quads x 1 000 rays, or the axis-aligned quad whose den and t are exact functions of
    the ray) through rt_quad_prepare / rt_quad_hit / rt_quad_normal against tests/quad_mini.py: accept decision, t, P, normal, front_face"""
    total = hits = 0
    for quv, rays, closest in class_tables(cls):
        with np.errstate(all="ignore"):
            hits += _compare(quad_sim, quv, rays, closest, cls)
        total += len(rays)
    assert total >= 100_000
    print(f"{cls}: {hits} of {total} rays hit")
    if cls not in ("magnitudes", "non_finite", "on_plane"):
        assert 0.05 * total < hits < 0.95 * total, "the class straddles the decision it is about"


def test_prepare_refuses_what_the_contract_refuses(quad_sim):
    quv = np.array([
        [0, 0, 0, 1, 0, 0, 0, 1, 0], [np.nan, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, np.inf, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0, 0, -np.inf, 0],
        [0, 0, 0, 1, 0, 0, 2, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 1e-160, 0, 0, 0, 1e-160, 0], [0, 0, 0, 1e160, 0, 0, 0, 1e160, 0],
        [0, 0, 0, 1.5e-154, 0, 0, 0, 1.0, 0], [0, 0, 0, 1.4e-154, 0, 0, 0, 1.0, 0], [1e308, 0, 0, 1e100, 0, 0, 0, 1e50, 0]], np.float64)
    rec, st = quad_sim.quad_prepare_v(quv)
    assert st.tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 0, 2, 0]      # (1.5e-154^2 = 2.25e-308 is normal, 1.4e-154^2 = 1.96e-308 is not)
    for row, s, r in zip(quv, st, rec):
        c = QM.QuadConsts(row[0:3], row[3:6], row[6:9])
        assert c.ok == (s == 0)
        if c.ok:
            assert _bits(r).tolist() == _bits(list(c.Q) + list(c.u) + list(c.v) + list(c.N) + list(c.w) + [c.D]).tolist()
    # the box's six quads, with the header's operations
    mn, mx = np.array([0.1, -0.7, 0.3]), np.array([0.4, 0.2, 1.1])
    out = quad_sim.quad_box(mn, mx)
    want = np.array([list(a) + list(b) + list(c) for a, b, c in QM.box_quads(mn, mx)])
    assert _bits(out).tolist() == _bits(want).tolist()
    # all six normals point out of the box
    centre = (mn + mx) / 2
    for row in out:
        c = QM.QuadConsts(row[0:3], row[3:6], row[6:9])
        mid = row[0:3] + 0.5 * row[3:6] + 0.5 * row[6:9]
        assert np.dot(np.array(c.N), mid - centre) > 0


def test_aimed_rays_hit_iff_the_target_is_inside(quad_sim):
    """Without the restatement.  A ray aimed at Q + a u + b v from either side hits iff 0 < a, b < 1, outside a margin of 1e-9 around the
    edges.  The margin comes from an f64 error bound (u = 2^-53 = 1.1e-16) for the worlds drawn here: |Q_c| <= 8; 0.5 <= |u|, |v| <= 4 with
    at least 30 degrees between them; -0.5 <= a, b <= 1.5, so |p| <= 12, |target| < 26; the origin 0.5 .. 16 from the target (|o| < 42) and
    at least 0.1 rad off the plane.
      * the target as numpy forms it lies within 4 roundings of magnitudes below 2^5 of the exact Q + a u + b v: < 3e-14 in space; d =
        (target - o) s carries two roundings, so the line misses the target by < 2 u * 16 < 4e-15;
      * t = (D - N.o) / den: N, D = N.Q and N.o carry fewer than 20 roundings of magnitudes below |Q|, |o| < 42: the numerator — the
        distance of o from the plane — is off by < 4e-14 (+ N's own 3 u of direction over |o - Q| < 50: 2e-14).  Along the ray that is
        |d| dt = (numerator error) / sin(incidence) < 6e-14 / sin(0.1) < 6.1e-13; P = o + d t adds two roundings below 64: 1.4e-14;
      * alpha = w . (p x v): its gradient in p is at most |w| |v| = 1 / (|u| sin(angle)) <= 4, and evaluating it takes about 12 roundings of
        magnitudes below |w| |p| |v| <= |p| / (|u| sin(angle)) <= 48: 6.4e-14 (w's own 3 u: 2e-14).
    Together < 4 * (6.1e-13 + 1.4e-14 + 3e-14 + 4e-15) + 8.4e-14 < 3e-12 on alpha and on beta: the margin of 1e-9 leaves a factor of 300."""
    rng = np.random.default_rng(2100)
    margin = 1e-9
    done = sides = 0
    while done < 200:
        def edge():
            e = rng.standard_normal(3)
            return e / np.linalg.norm(e) * rng.uniform(0.5, 4.0)
        u, v = edge(), edge()
        if abs(np.dot(u, v)) / (np.linalg.norm(u) * np.linalg.norm(v)) > math.cos(math.radians(30.0)):
            continue
        quv = np.concatenate([rng.uniform(-8.0, 8.0, 3), u, v])
        n_r = 600
        ab = rng.uniform(-0.5, 1.5, (n_r, 2))
        near = rng.random((n_r, 2)) < 0.4         # many targets just inside / just outside an edge
        side = np.where(rng.random((n_r, 2)) < 0.5, 0.0, 1.0)
        off = 10.0 ** rng.uniform(-9, -3, (n_r, 2)) * np.where(rng.random((n_r, 2)) < 0.5, 1.0, -1.0)
        ab = np.where(near, side + off, ab)
        rays = _aimed(rng, quv, n_r, ab)
        nrm = np.cross(u, v)
        nrm /= np.linalg.norm(nrm)
        dirs = rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1)[:, None]
        keep = np.abs(dirs @ nrm) >= math.sin(0.1)
        st, hit, t, P, _, front = quad_sim.quad_hit_v(quv, rays, np.full(n_r, 1.7976931348623157e308))
        assert st == 0
        inside = ((ab > margin) & (ab < 1.0 - margin)).all(axis=1)
        outside = ((ab < -margin) | (ab > 1.0 + margin)).any(axis=1)
        assert (hit[keep & inside] == 1).all() and (hit[keep & outside] == 0).all(), quv
        assert (front[keep & inside] == (dirs @ nrm < 0)[keep & inside]).all(), "both sides are hit, and front_face tells them apart"
        sides += int(0 < front[keep & inside].sum() < (keep & inside).sum())
        done += 1
    assert sides > 190


def test_swapped_winding_gives_the_same_hit(quad_sim):
    """Without the restatement.  (Q, v, u) against (Q, u, v): n, N, D, w and den change sign — every step an exact negation — so the accept
    decision, t, P and the hit normal keep their bits (front_face flips; alpha and beta change places)."""
    rng = np.random.default_rng(2101)
    total = 0
    for kind in ("generic", "skewed", "needle"):
        for quv in _quads(rng, 40, kind):
            rays = _aimed(rng, quv, 500)
            closest = np.where(rng.random(500) < 0.5, 1.7976931348623157e308, rng.uniform(0.0, 8.0, 500))
            a = quad_sim.quad_hit_v(quv, rays, closest)
            b = quad_sim.quad_hit_v(np.concatenate([quv[0:3], quv[6:9], quv[3:6]]), rays, closest)
            assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1])
            for x, y in zip(a[2:5], b[2:5]):
                assert np.array_equal(_bits(x), _bits(y)), kind
            assert np.array_equal(a[5][a[1] == 1], 1 - b[5][b[1] == 1])
            total += int(a[1].sum())
    assert total > 10_000


# ------------------------------------------------------------------ the tables
def _c_quad(abi, q=(-1.0, 0.0, -1.0), u=(2.0, 0.0, 0.0), v=(0.0, 0.0, 2.0), kind=0, **kw):
    r = abi.RtQuad()
    r.q[:] = q; r.u[:] = u; r.v[:] = v
    r.albedo[:] = [0.5, 0.5, 0.5]
    r.kind, r.h_offset, r.tex_w, r.tex_h, r.tex_id, r.fuzz_or_ior = kind, 2.0, 7, 0, 0, 1.5
    for k, val in kw.items():
        setattr(r, k, val)
    return r


def _c_world(abi, n=30):
    spheres = (abi.RtSphere * n)()
    rng = np.random.default_rng(5)
    for i, s in enumerate(spheres):
        s.center[:] = [float(x) for x in rng.uniform(-4, 4, 3)]
        s.radius = 0.3
        s.albedo[:] = [0.5, 0.5, 0.5]
        s.kind = (abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_GLASS)[i % 3]
        s.fuzz_or_ior = 1.5
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=4, height=4, samples_per_pixel=1, max_depth=2, sky_mode=1, spheres=spheres, n_spheres=n)
    return sc, spheres


def _tables(L, sc, quads):
    return L.tables(sc, quads=(type(quads[0]) * len(quads))(*quads) if quads else None)


def test_tables_validate_quads_and_leave_the_spheres_tables_alone(abi, quad_sim):
    """through the C structs (what rt_hip_scene_create_quads sees): no quad builds the quad-free tables byte for byte; quads append their
    material records behind the spheres' and change no other table; bad records are refused with the quad's index"""
    sc, keep = _c_world(abi)
    free, info0, _ = _tables(quad_sim, sc, None)
    assert info0[4] == 0 and info0[5] == 1 and free[11] == b""
    # (a non-null pointer with a count of 0 is no quad either)
    one = (abi.RtQuad * 1)(_c_quad(abi))
    blob, info = quad_sim.tables_blob(sc, quads=one, n_quads=0)
    assert b"".join(len(p).to_bytes(8, "little") + p for p in free[:12]) + free[12] == blob
    quads = [_c_quad(abi), _c_quad(abi, kind=abi.RT_MAT_METAL), _c_quad(abi, kind=abi.RT_MAT_GLASS), _c_quad(abi, kind=abi.RT_MAT_CHECKER),
             _c_quad(abi, kind=abi.RT_MAT_NOISE, tex_id=2)]
    with_q, info, _ = _tables(quad_sim, sc, quads)
    n = sc.n_spheres
    assert info[4] == 5 and info[0] == 2 and info[5] == 0, "five quads, two of them solids; the QUADS kernels use the general colour map"
    for k in (0, 3, 4, 5, 6, 7, 8, 9, 10, 12):
        assert with_q[k] == free[k], k                 # geometry, the grid, `large`, motion, media, lights: untouched
    assert with_q[1][:80 * n] == free[1] and len(with_q[1]) == 80 * (n + 5) and with_q[2][:48 * n] == free[2] and len(with_q[2]) == 48 * (n + 5)
    assert len(with_q[11]) == 128 * 5
    rec = np.frombuffer(with_q[11], np.float64).reshape(5, 16)
    c = QM.QuadConsts((-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0))
    assert _bits(rec[0]).tolist() == _bits(list(c.Q) + list(c.u) + list(c.v) + list(c.N) + list(c.w) + [c.D]).tolist()
    kinds = np.frombuffer(with_q[2], np.uint32).reshape(n + 5, 12)[n:, 3]
    assert kinds.tolist() == [0, 1, 2, 6, 7]
    for kw, msg in ((dict(kind=abi.RT_MAT_TEXTURE), "Texture"), (dict(kind=abi.RT_MAT_LIGHT), "Light"), (dict(kind=abi.RT_MAT_MEDIUM), "Medium"), (dict(kind=8), "kind"),
                    (dict(q=(float("nan"), 0.0, 0.0)), "finite"), (dict(u=(float("inf"), 0.0, 0.0)), "finite"), (dict(v=(4.0, 0.0, 0.0)), "degenerate"),
                    (dict(u=(1e-160, 0.0, 0.0), v=(0.0, 1e-160, 0.0)), "degenerate"), (dict(u=(1e160, 0.0, 0.0), v=(0.0, 1e160, 0.0)), "degenerate"),
                    (dict(kind=abi.RT_MAT_CHECKER, h_offset=0.0), "scale"), (dict(kind=abi.RT_MAT_NOISE, h_offset=float("inf")), "scale"),
                    (dict(kind=abi.RT_MAT_NOISE, tex_w=0), "octaves"), (dict(kind=abi.RT_MAT_NOISE, tex_w=17), "octaves"),
                    (dict(kind=abi.RT_MAT_NOISE, tex_id=3), "mode"), (dict(kind=abi.RT_MAT_NOISE, tex_h=1 << 32), "seed")):
        geo = {k: kw.pop(k) for k in ("q", "u", "v") if k in kw}
        parts, _, why = _tables(quad_sim, sc, [_c_quad(abi), _c_quad(abi, **geo, **kw)])
        assert parts is None and "quad 1" in why and msg in why, (kw, why)


def test_ids_and_ties(abi, oracle, quad_sim):
    """quad k is object n_spheres + k; on an equal t a sphere beats a quad and an earlier quad a later one.  A sphere of radius 1 at
    (0, 1, 0) touches the plane y = 0 at the origin: the ray from (0, -3, 0) along +y meets both at t = 3 exactly (sphere: half_b = -4,
    c = 15, disc = 1, root 4 - 1; quad: D = 0, N.o = 3, den = -1).  Two coincident quads: the first is kept."""
    spheres = (abi.RtSphere * 2)()
    spheres[0].center[:] = [5.0, 5.0, 5.0]; spheres[0].radius = 0.5
    spheres[1].center[:] = [0.0, 1.0, 0.0]; spheres[1].radius = 1.0
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=4, height=4, samples_per_pixel=1, max_depth=2, sky_mode=1, spheres=spheres, n_spheres=2)
    floor = _c_quad(abi, (-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0))
    quads = (abi.RtQuad * 3)(_c_quad(abi, (-2.0, -1.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0)), floor, floor)
    rays = np.array([[0.0, -3.0, 0.0, 0.0, 1.0, 0.0],      # the tie of sphere 1 and quads 1, 2 (quad 0 lies at t = 2: it wins outright)
                     [0.0, -0.5, 0.0, 0.0, 1.0, 0.0],      # from between the planes: the tie at t = 0.5
                     [1.5, -0.5, 0.0, 0.0, 2.0, 0.0],      # beside the sphere: the coincident quads alone
                     [1.5, 3.0, 0.0, 0.0, -1.0, 0.0],      # from above: the coincident quads before quad 0
                     [5.0, 9.0, 5.0, 0.0, -1.0, 0.0],      # sphere 0, off every quad
                     [9.0, 9.0, 9.0, 0.0, 1.0, 0.0]])      # nothing
    rc, best, t, _ = quad_sim.hit_world_v(sc, rays, quads=quads, miss_t=0.0)
    assert rc == 0
    assert best.tolist() == [2 + 0, 1, 2 + 1, 2 + 1, 0, -1] and t[:4].tolist() == [2.0, 0.5, 0.25, 3.0]
    m = QM.QuadMini(sc, lambda y, x: oracle.lib(abi).rt_oracle_atan2(y, x), quads=list(quads))
    m.pixel = m.sample = 0
    for ray, b, tt in zip(rays.tolist(), best.tolist(), t.tolist()):
        hit = m.hit_world(tuple(ray[:3]), tuple(ray[3:]), 0)
        assert (hit[0] if hit else -1) == b and (hit is None or m.last_t == tt)
    # without the sphere the quad is what the first two rays see
    sc.n_spheres = 1
    rc, best, t, _ = quad_sim.hit_world_v(sc, rays[:2], quads=quads, miss_t=0.0)
    assert rc == 0
    assert best[:2].tolist() == [1 + 0, 1 + 1] and t[:2].tolist() == [2.0, 0.5]


def test_the_black_occluders_geometry(abi):
    """the condition of tests/test_quad_gpu.py::test_black_occluder, confirmed with the restatement: with any jitter in [0, 1) every ray of
    a column left of c hits the quad, every ray of a column right of c misses it (the hit is monotone in the abscissa: the extremes of
    the jitter decide), and column c itself is split"""
    import test_quad_gpu as G
    sc, keep, quads = G.occluder_scene(abi, True)
    c = QM.QuadConsts(tuple(quads[0].q), tuple(quads[0].u), tuple(quads[0].v))
    org, ll, hor, ver = (tuple(v) for v in (sc.cam_origin, sc.cam_lower_left, sc.cam_horizontal, sc.cam_vertical))
    last = 1.0 - 2.0 ** -53
    for x in range(G.OCC_W):
        got = set()
        for jx in (0.0, last):
            for y in (0, G.OCC_H - 1):
                for jy in (0.0, last):
                    u = (float(x) + jx) / (float(G.OCC_W) - 1.0)
                    v = (float(G.OCC_H) - (float(y) + jy)) / (float(G.OCC_H) - 1.0)
                    d = tuple(ll[k] + hor[k] * u + ver[k] * v - org[k] for k in range(3))
                    got.add(QM.quad_test(c, org, d, 1.7976931348623157e308) is not None)
        assert got == ({True} if x < G.OCC_C else ({False} if x > G.OCC_C else {True, False})), x


# ------------------------------------------------------------------ the QUADS lane code built for the host
SIM_CASES = [("floor", 8), ("floor", 50), ("room", 8), ("moving", 8), ("medium", 8), ("solid", 8), ("glass", 8), ("mirror", 8)]


@pytest.mark.parametrize("case,depth", SIM_CASES)
def test_cpu_build_of_the_lane_code_equals_the_restatement(abi, oracle, host, quad_sim, case, depth):
    """rt_core.h's QUADS lane code built for the host (quads_hit behind hit_world_grid, lane_shade<MEDIUM, true, true>: the SOLID arm whatever
    the scene holds, see tests/lanesim/lane_sim.h) against QuadMini on the pinhole frames of the GPU parity test (48 x 32 at spp 4):
    tests/parity.py's bar and the exact segment identity"""
    import test_quad_gpu as G
    from parity import assert_parity, pooled_atol
    sc, c1, lens, quads = G.parity_world(host, case, depth)
    rc, rgb, lin, segs = quad_sim.render(sc.ptr, c1, quads, features_or=quad_sim.F_SOLID)
    assert rc == 0 and rgb.shape == (G.H, G.W, 3)
    m_rgb, m_lin, m_segs, m_disc = G.mini_frame(oracle, abi, host, case, depth)
    assert_parity(rgb, lin, m_rgb, m_lin, case, atol=pooled_atol(G.SPP))
    assert segs == m_segs - m_disc, (segs, m_segs, m_disc)
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 100


@pytest.mark.parametrize("case", ["floor", "solid", "moving", "medium"])
def test_cpu_build_of_the_aovs_and_the_surface_record_equal_the_restatement(abi, oracle, host, quad_sim, case):
    import test_quad_gpu as G
    sc, c1, lens, quads = G.parity_world(host, case, 8)
    rc, got = quad_sim.aovs(sc.ptr, 2, c1, quads, features_or=quad_sim.F_SOLID)
    assert rc == 0 and got.shape == (G.H, G.W, 8)
    m = G._mini(oracle, abi, sc, c1, None, quads)
    want = m.aovs(2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    rc, rec = quad_sim.surface(sc.ptr, c1, quads)
    assert rc == 0 and rec.shape == (G.H, G.W)
    ids, kinds, ts = rec["id"], rec["kind"], rec["t"]
    w_ids, w_kinds, w_ts = m.surface()
    assert np.array_equal(ids, w_ids) and np.array_equal(kinds, w_kinds) and np.array_equal(_bits(ts), _bits(w_ts))
    n = sc.c.n_spheres
    assert ((ids >= n) & (ids < n + len(quads))).any() and (ids < n).any()
    if case == "solid":    # both colours of the checker floor show as albedo: the pattern is evaluated (in the quad's frame)
        floor = got[..., 0][ids == n + 0]
        assert floor.max() > 0.85 and floor.min() < 0.25
