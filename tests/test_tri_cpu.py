"""Triangles and meshes without a GPU: the schema (three spellings, their errors, the round trip, the example), rt_flat_hit built
for the host (tests/trisim) against the restatement of tests/tri_mini.py bit for bit, lim = 2 against rt_quad_hit bit for bit, a tiling
property that needs no restatement, the limit table rt_tables.h builds, ids and ties across shapes, and the CPU build of the QUADS lane code
(tests/lanesim, unchanged: DevScene::quads carries the limits through its call) against TriMini on the GPU test's pinhole frames."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import lane_sim
import quad_mini as QM
import tri_mini as TM
import tri_sim
from quad_rays import CLASSES, T_MAX, class_tables
from tri_rays import HYP_QUV, TRI_CLASSES, exact_rays, tri_class_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_SCENE = os.path.join(ROOT, "scenes", "cornell_mesh_600x600_spp128.json")
LAM = '{"Lambertian":{"albedo":[0.5,0.25,0.75]}}'
MET = '{"Metal":{"albedo":[0.9,0.8,0.7],"fuzz":0.125}}'
SPHERE = '{"center":{"x":0.0,"y":1.0,"z":0.0},"radius":0.5,"material":{"Glass":{"index_of_refraction":1.5}}}'
QUAD = '{"q":{"x":-1.0,"y":0.0,"z":-1.0},"u":{"x":2.0,"y":0.0,"z":0.25},"v":{"x":0.0,"y":0.5,"z":2.0},"material":%s}'
BOX = '{"box":{"min":[0.5,-1.0,2.0],"max":[1.5,0.25,4.0]},"material":' + MET + '}'
VERTS = [[0.1, 0.0, 0.3], [1.7, 0.2, 0.0], [0.3, 1.9, 0.1], [0.2, 0.4, 2.3]]
FACES = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]


def _cfg(*objects):
    return ('{"width":8,"height":8,"samples_per_pixel":1,"max_depth":2,"sky":{"texture":""},"camera":{"look_from":{"x":0.0,"y":1.0,"z":5.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":0.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":40.0,"aspect":1.0},"objects":[' + ",".join(objects) + ']}')


def _pt(p):
    return '{"x":%r,"y":%r,"z":%r}' % tuple(float(x) for x in p)


def _flat(q, u, v, shape, mat=LAM):
    return '{"q":%s,"u":%s,"v":%s,%s"material":%s}' % (_pt(q), _pt(u), _pt(v), '"shape":"%s",' % shape if shape else "", mat)


def _tri(a, b, c, mat=LAM):
    return '{"triangle":%s,"material":%s}' % (json.dumps([list(a), list(b), list(c)]), mat)


def _mesh(verts, faces, mat=LAM):
    return '{"mesh":{"vertices":%s,"faces":%s},"material":%s}' % (json.dumps(verts), json.dumps(faces), mat)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def sim():
    return tri_sim.load()


@pytest.fixture(scope="module")
def lanes(abi):
    return lane_sim.load(abi)


# ------------------------------------------------------------------ 1. schema
def test_schema_three_spellings_their_order_and_the_round_trip(host, abi):
    assert (abi.RT_QUAD_SHAPE_PARALLELOGRAM, abi.RT_QUAD_SHAPE_TRIANGLE) == (0, 1) and abi.RT_ABI_VERSION == 5 and C.sizeof(abi.RtQuad) == 128
    a, b, c = (0.1, -0.0, 1e-3), (3.0000000000000004, 0.5, 0.0), (0.25, 1e10, 0.7)
    sc = host.Scene.loads(_cfg(_tri(a, b, c), SPHERE, QUAD % LAM, _mesh(VERTS, FACES, MET), BOX, _flat((0, 0, 0), (1, 0, 0), (0, 1, 0), "triangle"),
                               _flat((0, 0, 1), (1, 0, 0), (0, 1, 0), "parallelogram"), SPHERE))
    q = sc.quads()
    assert sc.c.n_spheres == 2 and len(q) == 1 + 1 + 4 + 6 + 1 + 1
    assert [x.reserved for x in q] == [1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0], "file order, interleaved with spheres, quads and a box"
    # {"triangle": [a, b, c]}: Q = a, u = b - a, v = c - a, one subtraction per component
    want = TM.tri_from_corners(a, b, c)
    assert (tuple(q[0].q), tuple(q[0].u), tuple(q[0].v)) == want and math.copysign(1.0, q[0].q[1]) == -1.0
    assert q[0].kind == abi.RT_MAT_LAMBERTIAN and list(q[0].albedo) == [0.5, 0.25, 0.75]
    # a mesh: its triangles in face order, each with the mesh's material
    for k, t in enumerate(TM.mesh_triangles(VERTS, FACES)):
        m = q[2 + k]
        assert (tuple(m.q), tuple(m.u), tuple(m.v)) == t and m.kind == abi.RT_MAT_METAL and m.fuzz_or_ior == 0.125, k
    # ... equals its explicit triangles, in either explicit spelling, bit for bit
    tris = [_tri(VERTS[i], VERTS[j], VERTS[k], MET) for i, j, k in FACES]
    flats = [_flat(t[0], t[1], t[2], "triangle", MET) for t in TM.mesh_triangles(VERTS, FACES)]
    for explicit in (tris, flats):
        sc2 = host.Scene.loads(_cfg(_tri(a, b, c), SPHERE, QUAD % LAM, *explicit, BOX, _flat((0, 0, 0), (1, 0, 0), (0, 1, 0), "triangle"),
                                    _flat((0, 0, 1), (1, 0, 0), (0, 1, 0), None), SPHERE))
        assert bytes(sc2.quads()) == bytes(q) and sc2.to_json() == sc.to_json()
    # rt_scene_to_json writes the canonical form in the file's interleaving and round-trips every RtQuad bit for bit
    text = sc.to_json()
    objs = json.loads(text)["objects"]
    assert ["q" in o for o in objs] == [True, False] + [True] * 13 + [False] and not any(k in o for o in objs for k in ("box", "mesh", "triangle"))
    assert [o.get("shape") for o in objs if "q" in o] == ["triangle" if x.reserved else None for x in q]
    again = host.Scene.loads(text)
    assert again.to_json() == text and bytes(again.quads()) == bytes(q)
    assert [bytes(again.c.spheres[i]) for i in range(2)] == [bytes(sc.c.spheres[i]) for i in range(2)]
    # a file without a triangle serialises as it always did: no "shape" anywhere
    plain = host.Scene.loads(_cfg(QUAD % LAM, SPHERE, BOX))
    assert '"shape"' not in plain.to_json() and all(x.reserved == 0 for x in plain.quads())


BAD = [
    (_flat((0, 0, 0), (1, 0, 0), (0, 1, 0), "circle"), "unknown shape `circle`"),
    ('{"q":[0,0,0],"u":[1,0,0],"v":[0,1,0],"shape":3,"material":' + LAM + '}', "shape"),
    (_mesh(VERTS, [[0, 1, 2], [0, 1]]), "mesh face 1: a face has exactly three indices"),
    (_mesh(VERTS, [[0, 1, 2, 3]]), "mesh face 0: a face has exactly three indices"),
    (_mesh(VERTS, [[0, 1, 2], [0, 1, 4]]), "mesh face 1: index 4 out of range"),
    (_mesh(VERTS, [[0, 1, -1]]), "mesh face 0"),
    (_mesh(VERTS, [[0, 1, 1.5]]), "mesh face 0"),
    (_mesh(VERTS, [[0, 1, "2"]]), "mesh face 0"),
    ('{"mesh":{"vertices":[[0,0,0],[1,0,0],[0,1e999,0]],"faces":[[0,1,2]]},"material":' + LAM + '}', "mesh vertex 2"),
    ('{"triangle":[[0,0,0],[1,0,0],[0,1e999,0]],"material":' + LAM + '}', "number out of range"),
    ('{"triangle":[[-1e308,0,0],[1e308,0,0],[0,1,0]],"material":' + LAM + '}', "not finite"),
    (_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], [[0, 1, 2], [0, 1, 3]]), "mesh face 1: degenerate (collinear) triangle"),
    (_mesh(VERTS, [[0, 1, 2], [1, 1, 2]]), "mesh face 1: degenerate (collinear) triangle"),
    (_tri((0, 0, 0), (1, 1, 1), (2, 2, 2)), "degenerate (collinear) triangle"),
    (_flat((0, 0, 0), (1, 0, 0), (2, 0, 0), "triangle"), "degenerate (collinear) triangle"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0))[:-1] + ',"center":{"x":0,"y":0,"z":0}}', "mixed keys"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0))[:-1] + ',"q":{"x":0,"y":0,"z":0}}', "mixed keys"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0))[:-1] + ',"shape":"triangle"}', "mixed keys"),
    (_mesh(VERTS, FACES)[:-1] + ',"radius":1.0}', "mixed keys"),
    (_mesh(VERTS, FACES)[:-1] + ',"triangle":[[0,0,0],[1,0,0],[0,1,0]]}', "mixed keys"),
    (_mesh(VERTS, FACES)[:-1] + ',"box":{"min":[0,0,0],"max":[1,1,1]}}', "mixed keys"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0))[:-1] + ',"triangle":[[0,0,0],[1,0,0],[0,1,0]]}', "duplicate field `triangle`"),
    (_mesh(VERTS, FACES)[:-1] + ',"material":' + LAM + '}', "duplicate field `material`"),
    ('{"mesh":{"vertices":[[0,0,0]],"faces":[],"faces":[]},"material":' + LAM + '}', "duplicate field `faces`"),
    (_flat((0, 0, 0), (1, 0, 0), (0, 1, 0), "triangle")[:-1] + ',"shape":"triangle"}', "duplicate field `shape`"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0))[:-1] + ',"center1":{"x":0,"y":1,"z":0}}', "center1"),
    (_mesh(VERTS, FACES)[:-1] + ',"center1":{"x":0,"y":1,"z":0}}', "center1"),
    (_flat((0, 0, 0), (1, 0, 0), (0, 1, 0), "triangle")[:-1] + ',"center1":{"x":0,"y":1,"z":0}}', "center1"),
    ('{"triangle":[[0,0,0],[1,0,0]],"material":' + LAM + '}', "three vertices"),
    ('{"mesh":{"vertices":[[0,0,0]]},"material":' + LAM + '}', "missing field `faces`"),
    ('{"triangle":[[0,0,0],[1,0,0],[0,1,0]]}', "missing field `material`"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0), '{"Light":{}}'), "cannot be a Light"),
    (_mesh(VERTS, FACES, '{"Medium":{"albedo":[0.5,0.5,0.5],"density":1.0}}'), "cannot be a Medium"),
    (_tri((0, 0, 0), (1, 0, 0), (0, 1, 0), '{"Texture":{"albedo":[1,1,1],"pixels":"scenes/data/earth.jpg","width":8,"height":8,"h_offset":0.0}}'), "cannot be a Texture"),
]


@pytest.mark.parametrize("obj,msg", BAD)
def test_schema_errors_name_the_object_by_the_files_index(host, obj, msg):
    """the bad object is objects[2] of the file — behind a mesh (four entries) and a sphere, so no count of entries names it"""
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_cfg(_mesh(VERTS, FACES), SPHERE, obj))
    assert "objects[2]" in str(e.value) and msg in str(e.value), str(e.value)


def test_more_than_1024_entries_in_a_file_are_unsupported(host, abi):
    """RT_MAX_QUADS counts both shapes and what a mesh or a box expands to: 1024 load, the 1025th entry is RT_ERR_UNSUPPORTED and names its object"""
    faces = [[0, 1, 2]] * 509
    ok = host.Scene.loads(_cfg(_mesh(VERTS, faces), BOX, QUAD % LAM, _mesh(VERTS, faces[:508])))
    assert len(ok.quads()) == 1024
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_cfg(_mesh(VERTS, faces), BOX, QUAD % LAM, _mesh(VERTS, faces)))
    assert e.value.code == abi.RT_ERR_UNSUPPORTED and "objects[3]" in str(e.value) and "1024" in str(e.value), str(e.value)


def test_the_example_scene_is_generated(host, abi):
    spec = importlib.util.spec_from_file_location("make_cornell_mesh_scene", os.path.join(ROOT, "scenes", "make_cornell_mesh_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make() == open(MESH_SCENE).read()
    sc = host.Scene.load(MESH_SCENE)
    q = sc.quads()
    assert len(q) == 39 and sum(x.reserved for x in q) == 34 and [x.reserved for x in q[:5]] == [0] * 5
    kinds = [x.kind for x in q[5:]]
    assert kinds == [abi.RT_MAT_LAMBERTIAN] * 6 + [abi.RT_MAT_GLASS] * 8 + [abi.RT_MAT_METAL] * 20
    assert sc.c.n_spheres == 1 and sc.c.spheres[0].kind == abi.RT_MAT_LIGHT and sc.c.sky_mode == abi.RT_SKY_NONE
    assert (sc.c.width, sc.c.height, sc.c.samples_per_pixel, sc.c.max_depth) == (600, 600, 128, 50)
    # every mesh is closed and wound outward: each edge is used once in each direction, and every N points away from the mesh's centre
    for lo, hi in ((5, 11), (11, 19), (19, 39)):
        corners = [(tuple(x.q), tuple(x.q[k] + x.u[k] for k in range(3)), tuple(x.q[k] + x.v[k] for k in range(3))) for x in q[lo:hi]]
        snap = lambda p: tuple(round(v, 6) for v in p)
        edges = [(snap(t[i]), snap(t[(i + 1) % 3])) for t in corners for i in range(3)]
        assert len(set(edges)) == len(edges) and all((b, a) in set(edges) for a, b in edges)
        pts = np.array(sorted({snap(p) for t in corners for p in t}))
        centre = pts.mean(axis=0)
        for x, t in zip(q[lo:hi], corners):
            c = QM.QuadConsts(tuple(x.q), tuple(x.u), tuple(x.v))
            assert np.dot(np.array(c.N), np.mean(np.array(t), axis=0) - centre) > 0


# ------------------------------------------------------------------ 2. rt_flat_hit built for the host
def _compare(L, quv, rays, closest, what):
    """the host build (lim = 1) against tri_mini on every ray: accept decision, t, P, normal and front_face bit for bit; returns the hit count"""
    st, hit, t, P, nrm, front = L.flat_hit_v(quv, 1.0, rays, closest)
    c = QM.QuadConsts(quv[0:3], quv[3:6], quv[6:9])
    assert (st == 0) == c.ok, (what, quv)
    if not c.ok:
        return 0
    n_hit = 0
    tb, Pb, nb = _bits(t), _bits(P), _bits(nrm)
    for i, (ray, cl) in enumerate(zip(rays.tolist(), closest.tolist())):
        r = TM.flat_test(c, 1.0, ray[0:3], ray[3:6], cl)
        if r is None:
            assert not hit[i], (what, quv, ray, cl)
            continue
        n_hit += 1
        f, nm = QM.quad_record(c, ray[3:6])
        assert hit[i] and bool(front[i]) == f, (what, quv, ray, cl)
        assert tb[i] == _bits([r[0]])[0] and Pb[i].tolist() == _bits(r[1]).tolist() and nb[i].tolist() == _bits(nm).tolist(), (what, quv, ray, cl)
    return n_hit


@pytest.mark.filterwarnings("ignore::RuntimeWarning")     # (the classes make NaN, inf and overflow on purpose)
@pytest.mark.parametrize("cls", TRI_CLASSES)
def test_host_build_equals_the_restatement_bit_for_bit(sim, cls):
    """>= 10^5 rays per class (tests/tri_rays.py: the nine quad classes read as triangles, and `hypotenuse`) through rt_quad_prepare /
    rt_flat_hit(lim = 1) / rt_quad_normal against tests/tri_mini.py: accept decision, t, P, normal, front_face"""
    total = hits = 0
    for quv, rays, closest in tri_class_tables(cls):
        with np.errstate(all="ignore"):
            hits += _compare(sim, quv, rays, closest, cls)
        total += len(rays)
    assert total >= 100_000
    print(f"{cls}: {hits} of {total} rays hit the triangle")
    if cls == "hypotenuse":
        assert 0.25 * total < hits < 0.75 * total, "the class straddles the decision it is about"
    elif cls not in ("magnitudes", "non_finite", "on_plane"):
        assert 0.02 * total < hits < 0.95 * total


def test_the_exact_hypotenuse(sim):
    """Without the restatement: against HYP_QUV alpha and beta are exact functions of the ray (tests/tri_rays.py).  alpha + beta == 1 exactly is
    accepted — (1/2, 1/2), (1/4, 3/4), every (j / 1024, 1 - j / 1024), the corners (1, 0) and (0, 1); one ulp of the sum further out is
    rejected; one ulp further in is accepted; the parallelogram accepts all of them."""
    a = np.arange(0, 1025) / 1024.0
    free = np.full(len(a), T_MAX)
    on = exact_rays(a, 1.0 - a)
    assert sim.flat_hit_v(HYP_QUV, 1.0, on, free)[1].tolist() == [1] * 1025
    m = a[1:-1]
    out = exact_rays(m, (1.0 - m) + 2.0 ** -52)       # beta in [2^-10, 1): + 2^-52 is exact, and alpha + beta = 1 + 2^-52 exactly
    assert not sim.flat_hit_v(HYP_QUV, 1.0, out, free[:len(m)])[1].any()
    inn = exact_rays(m, (1.0 - m) - 2.0 ** -53)       # alpha + beta = 1 - 2^-53 exactly
    assert sim.flat_hit_v(HYP_QUV, 1.0, inn, free[:len(m)])[1].all()
    for rays in (on, out, inn):
        assert sim.flat_hit_v(HYP_QUV, 2.0, rays, free[:len(rays)])[1].all() and sim.quad_hit_v(HYP_QUV, rays, free[:len(rays)])[1].all()
    # the sum is ONE rounded addition: alpha = 2^-1, beta = 2^-1 + 2^-53 sums to 1 + 2^-53, which rounds (to even) to 1: accepted
    tie = exact_rays(np.array([0.5]), np.array([0.5 + 2.0 ** -53]))
    assert sim.flat_hit_v(HYP_QUV, 1.0, tie, free[:1])[1].tolist() == [1]


# ------------------------------------------------------------------ 3. lim = 2 is the old test
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", CLASSES)
def test_limit_two_is_rt_quad_hit(sim, cls):
    """rt_flat_hit(rec, 2.0, ...) equals rt_quad_hit in decision and every output bit on all nine class tables of tests/quad_rays.py"""
    total = hits = 0
    for quv, rays, closest in class_tables(cls):
        with np.errstate(all="ignore"):
            a = sim.flat_hit_v(quv, 2.0, rays, closest)
            b = sim.quad_hit_v(quv, rays, closest)
        assert a[0] == b[0]
        if a[0]:
            continue
        assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3])), cls
        total += len(rays); hits += int(a[1].sum())
    assert total >= 70_000 and (hits > 0.05 * total or cls in ("magnitudes", "non_finite", "on_plane"))


# ------------------------------------------------------------------ 4. two triangles tile their parallelogram (no restatement)
def test_two_triangles_tile_the_parallelogram(sim):
    """(Q, u, v) and (Q + u + v, -u, -v) as triangles against (Q, u, v) as a parallelogram, for rays aimed at Q + a u + b v from either side: at
    least a margin away from the four edges and from the diagonal a + b = 1, exactly one triangle accepts iff the parallelogram accepts
    (the first iff a + b < 1), and outside the parallelogram none does.

    The margin.  The worlds are those of tests/test_quad_cpu.py::test_aimed_rays_hit_iff_the_target_is_inside (|Q_c| <= 8; 0.5 <= |u|, |v| <=
    4, at least 30 degrees apart; -0.5 <= a, b <= 1.5; the origin 0.5 .. 16 from the target and at least 0.1 rad off the plane), whose
    docstring bounds the error of the computed alpha and beta by 3e-12 each (u = 2^-53).  The second triangle's frame is Q' = (Q + u) + v:
    two more roundings of magnitudes below 16 (3.6e-15 in space, times the gradient |w| |v| <= 4: 1.5e-14), |Q'| <= 16 sqrt(3) < 42 stays
    inside the magnitudes that bound used, and |P - Q'| <= 12 as before: alpha', beta' (= 1 - alpha, 1 - beta exactly) carry < 3.1e-12 each.
    The sums alpha + beta and alpha' + beta' therefore carry < 6.2e-12 + one rounding of a sum below 2 (2.2e-16).  A margin of 1e-9 on
    each edge and on the diagonal leaves a factor of 160.

    The draw.  Directions are redrawn until they are 0.1 rad off the plane, and the near-edge and near-diagonal targets keep 1e-8 .. 1e-3
    away, so only targets that the uniform draw itself puts inside a margin are left out: at most 1 % (asserted; in fact about 1e-8)."""
    rng = np.random.default_rng(2110)
    margin = 1e-9
    drawn = left_out = ones = twos = 0
    done = 0
    while done < 200:
        def edge():
            e = rng.standard_normal(3)
            return e / np.linalg.norm(e) * rng.uniform(0.5, 4.0)
        u, v = edge(), edge()
        if abs(np.dot(u, v)) / (np.linalg.norm(u) * np.linalg.norm(v)) > math.cos(math.radians(30.0)):
            continue
        Q = rng.uniform(-8.0, 8.0, 3)
        quv = np.concatenate([Q, u, v])
        quv2 = np.concatenate([(Q + u) + v, -u, -v])
        n_r = 600
        ab = rng.uniform(-0.5, 1.5, (n_r, 2))
        off = 10.0 ** rng.uniform(-8, -3, (n_r, 2)) * np.where(rng.random((n_r, 2)) < 0.5, 1.0, -1.0)
        kind = rng.integers(0, 5, n_r)                      # 0, 1: uniform; 2: near an edge; 3, 4: near the diagonal
        side = np.where(rng.random((n_r, 2)) < 0.5, 0.0, 1.0)
        near_edge = (kind == 2)[:, None] & (rng.random((n_r, 2)) < 0.7)
        ab = np.where(near_edge, side + off, ab)
        a_d = rng.uniform(0.0, 1.0, n_r)
        ab = np.where((kind >= 3)[:, None], np.stack([a_d, (1.0 - a_d) + off[:, 0]], axis=1), ab)
        nrm = np.cross(u, v)
        nrm /= np.linalg.norm(nrm)
        target = Q + ab[:, :1] * u + ab[:, 1:] * v
        dirs = rng.standard_normal((n_r, 3))
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        while True:
            flat = np.abs(dirs @ nrm) < math.sin(0.1)
            if not flat.any():
                break
            new = rng.standard_normal((int(flat.sum()), 3))
            dirs[flat] = new / np.linalg.norm(new, axis=1)[:, None]
        o = target - dirs * rng.uniform(0.5, 16.0, (n_r, 1))
        rays = np.concatenate([o, (target - o) * rng.uniform(0.25, 4.0, (n_r, 1))], axis=1)
        free = np.full(n_r, T_MAX)
        st, par = sim.flat_hit_v(quv, 2.0, rays, free)[:2]
        st1, t1 = sim.flat_hit_v(quv, 1.0, rays, free)[:2]
        st2, t2 = sim.flat_hit_v(quv2, 1.0, rays, free)[:2]
        assert st == st1 == st2 == 0
        s = ab[:, 0] + ab[:, 1]
        clear = (np.abs(ab) > margin).all(axis=1) & (np.abs(ab - 1.0) > margin).all(axis=1) & (np.abs(s - 1.0) > margin)
        inside = ((ab > 0.0) & (ab < 1.0)).all(axis=1)
        drawn += n_r
        left_out += int((~clear).sum())
        assert np.array_equal(par[clear], inside[clear].astype(np.int32)), quv
        assert np.array_equal((t1 + t2)[clear], par[clear]), "exactly one triangle accepts iff the parallelogram accepts"
        assert np.array_equal(t1[clear], (inside & (s < 1.0))[clear].astype(np.int32)) and np.array_equal(t2[clear], (inside & (s > 1.0))[clear].astype(np.int32))
        ones += int(t1[clear].sum()); twos += int(t2[clear].sum())
        done += 1
    print(f"{drawn} rays, {left_out} inside a margin, {ones} on the first triangle, {twos} on the second")
    assert left_out <= 0.01 * drawn
    assert ones > 0.1 * drawn and twos > 0.1 * drawn


# ------------------------------------------------------------------ 5. the tables, through the C structs
def _c_flat(abi, q=(-1.0, 0.0, -1.0), u=(2.0, 0.0, 0.0), v=(0.0, 0.0, 2.0), shape=0, kind=0, **kw):
    r = abi.RtQuad()
    r.q[:] = q; r.u[:] = u; r.v[:] = v
    r.albedo[:] = [0.5, 0.5, 0.5]
    r.kind, r.h_offset, r.tex_w, r.tex_h, r.tex_id, r.fuzz_or_ior, r.reserved = kind, 2.0, 7, 0, 0, 1.5, shape
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


def test_tables_hold_a_limit_per_entry_only_when_there_is_a_triangle(abi, sim, lanes):
    """through the C structs (what rt_hip_scene_create_quads sees).  No triangle: no limit table, DevScene's limit pointer null, n_tris 0 — and
    every other table is, byte for byte, what the same entries build whatever their shapes (the parent's bytes: tests/test_quad_cpu.py pins
    them against the quad-free tables).  With triangles: 2.0 / 1.0 per entry, the records and materials unchanged.  Refusals name their entry."""
    sc, keep = _c_world(abi)
    kinds = [abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_GLASS, abi.RT_MAT_CHECKER, abi.RT_MAT_NOISE]
    shapes = [1, 0, 1, 1, 0]
    par = [_c_flat(abi, kind=k) for k in kinds]
    mix = [_c_flat(abi, kind=k, shape=s) for k, s in zip(kinds, shapes)]
    lim, info = sim.tables(sc, par)
    assert len(lim) == 0 and info.tolist() == [0, 0, 5, 0, 0]
    lim, info = sim.tables(sc, None)
    assert len(lim) == 0 and info.tolist() == [0, 0, 0, 0, 0]
    lim, info = sim.tables(sc, mix)
    assert lim.tolist() == [1.0, 2.0, 1.0, 1.0, 2.0] and info.tolist() == [5, 3, 5, 1, 3]
    arr = lambda qs: (abi.RtQuad * len(qs))(*qs)
    a, info_a, _ = lanes.tables(sc, quads=arr(par))
    b, info_b, _ = lanes.tables(sc, quads=arr(mix))
    assert a == b and info_a.tolist() == info_b.tolist(), "records, materials and every sphere table are the parallelograms'"
    assert len(a[11]) == 128 * 5
    for kw, msg in ((dict(shape=2), "bad shape"), (dict(shape=0xFFFFFFFF), "bad shape"), (dict(shape=1, kind=abi.RT_MAT_TEXTURE), "Texture"),
                    (dict(shape=1, kind=abi.RT_MAT_LIGHT), "Light"), (dict(shape=1, kind=abi.RT_MAT_MEDIUM), "Medium"), (dict(shape=1, kind=8), "kind"),
                    (dict(shape=1, q=(float("nan"), 0.0, 0.0)), "finite"), (dict(shape=1, v=(4.0, 0.0, 0.0)), "degenerate"),
                    (dict(shape=1, kind=abi.RT_MAT_CHECKER, h_offset=0.0), "scale"), (dict(shape=1, kind=abi.RT_MAT_NOISE, tex_w=17), "octaves")):
        got, why = sim.tables(sc, [_c_flat(abi, shape=1), _c_flat(abi, **kw)])
        assert got is None and "quad 1" in why and msg in why, (kw, why)


# ------------------------------------------------------------------ 6. ids and ties
def test_ids_and_ties_across_shapes(abi, oracle, lanes):
    """entry k is object n_spheres + k whatever its shape.  A triangle and a parallelogram in the plane y = 0, overlapping: the earlier entry
    wins, in both orders; where only one covers the point, that one; a sphere of radius 1 at (0, 1, 0) touches the plane at the origin and
    wins the exact tie at t = 3 (tests/test_quad_cpu.py::test_ids_and_ties has the arithmetic)."""
    spheres = (abi.RtSphere * 2)()
    spheres[0].center[:] = [5.0, 5.0, 5.0]; spheres[0].radius = 0.5
    spheres[1].center[:] = [0.0, 1.0, 0.0]; spheres[1].radius = 1.0
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=4, height=4, samples_per_pixel=1, max_depth=2, sky_mode=1, spheres=spheres, n_spheres=2)
    tri = _c_flat(abi, (-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), shape=1)        # covers x + z <= 0 of the square [-2, 2]^2
    par = _c_flat(abi, (-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), shape=0)
    rays = np.array([[0.0, -3.0, 0.0, 0.0, 1.0, 0.0],       # the tie of sphere 1 with both entries at t = 3: the sphere
                     [-1.0, -0.5, -0.5, 0.0, 1.0, 0.0],     # both cover (-1, -0.5): the earlier entry
                     [1.0, -0.5, 1.0, 0.0, 2.0, 0.0],       # only the parallelogram covers (1, 1)
                     [1.0, 3.0, -1.0, 0.0, -1.0, 0.0],      # ON the hypotenuse (x + z = 0, alpha + beta = 1 exactly), from above: both cover it
                     [3.0, -0.5, 0.0, 0.0, 1.0, 0.0]])      # beside both
    m_args = lambda quads: TM.TriMini(sc, lambda y, x: oracle.lib(abi).rt_oracle_atan2(y, x), quads=list(quads))
    for order, want in (((tri, par), [1, 2 + 0, 2 + 1, 2 + 0, -1]), ((par, tri), [1, 2 + 0, 2 + 0, 2 + 0, -1])):
        quads = (abi.RtQuad * 2)(*order)
        rc, best, t, _ = lanes.hit_world_v(sc, rays, quads=quads, miss_t=0.0)
        assert rc == 0 and best.tolist() == want and t[:4].tolist() == [3.0, 0.5, 0.25, 3.0], (best.tolist(), t.tolist())
        m = m_args(quads)
        m.pixel = m.sample = 0
        for ray, b, tt in zip(rays.tolist(), best.tolist(), t.tolist()):
            hit = m.hit_world(tuple(ray[:3]), tuple(ray[3:]), 0)
            assert (hit[0] if hit else -1) == b and (hit is None or m.last_t == tt)
    # a triangle listed first does not shadow a parallelogram behind the hypotenuse, and a lone triangle misses there
    rc, best, _, _ = lanes.hit_world_v(sc, rays[2:3], quads=(abi.RtQuad * 1)(tri), miss_t=0.0)
    assert rc == 0 and best.tolist() == [-1]


# ------------------------------------------------------------------ 7. the QUADS lane code built for the host
SIM_CASES = [("tetra", 8), ("tetra", 50), ("room", 8), ("glass", 8), ("metal", 8), ("medium", 8), ("solid", 8), ("coincident", 8)]


@pytest.mark.parametrize("case,depth", SIM_CASES)
def test_cpu_build_of_the_lane_code_equals_the_restatement(abi, oracle, host, lanes, case, depth):
    """rt_core.h's QUADS lane code built for the host — quads_hit with the limit table behind hit_world_grid, through the unchanged call of
    tests/lanesim/lane_sim.h — against TriMini on the pinhole frames of the GPU parity test (48 x 32 at spp 4): tests/parity.py's bar and
    the exact segment identity"""
    import test_tri_gpu as G
    from parity import assert_parity, pooled_atol
    sc, c1, lens, quads = G.parity_world(host, case, depth)
    assert any(q.reserved for q in quads)
    rc, rgb, lin, segs = lanes.render(sc.ptr, c1, quads)
    assert rc == 0 and rgb.shape == (G.H, G.W, 3)
    m_rgb, m_lin, m_segs, m_disc = G.mini_frame(oracle, abi, host, case, depth)
    assert_parity(rgb, lin, m_rgb, m_lin, case, atol=pooled_atol(G.SPP))
    assert segs == m_segs - m_disc, (segs, m_segs, m_disc)
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 100


@pytest.mark.parametrize("case", ["tetra", "solid", "medium", "coincident"])
def test_cpu_build_of_the_aovs_and_the_surface_record_equal_the_restatement(abi, oracle, host, lanes, case):
    import test_tri_gpu as G
    sc, c1, lens, quads = G.parity_world(host, case, 8)
    rc, got = lanes.aovs(sc.ptr, 2, c1, quads)
    assert rc == 0 and got.shape == (G.H, G.W, 8)
    m = G._mini(oracle, abi, sc, c1, None, quads)
    want = m.aovs(2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    rc, rec = lanes.surface(sc.ptr, c1, quads)
    assert rc == 0 and rec.shape == (G.H, G.W)
    w_ids, w_kinds, w_ts = m.surface()
    assert np.array_equal(rec["id"], w_ids) and np.array_equal(rec["kind"], w_kinds) and np.array_equal(_bits(rec["t"]), _bits(w_ts))
    n = sc.c.n_spheres
    tri_ids = [n + k for k, q in enumerate(quads) if q.reserved]
    assert np.isin(w_ids, tri_ids).sum() > 20, "triangles are first hits of the frame"
    if case == "coincident":   # the earlier entry shows where the three overlap: ids in file order n + 0 (triangle), n + 1 (quad), n + 2 (triangle)
        assert all((w_ids == n + k).sum() > 10 for k in range(3))
        # ... and reading the triangles as parallelograms gives another record
        as_par = (abi.RtQuad * len(quads))(*quads)
        for q in as_par:
            q.reserved = 0
        rc, other = lanes.surface(sc.ptr, c1, as_par)
        assert rc == 0 and (other["id"] != rec["id"]).sum() > 10


def test_two_triangle_floor_on_the_cpu_build(abi, host, lanes):
    """the condition of tests/test_tri_gpu.py::test_two_triangles_are_their_parallelogram, confirmed on the CPU build first: the frame, the
    segment count and the surface record's t of the floor as one parallelogram and as its two triangles agree bit for bit — no ray of these
    frames falls into a crack on the diagonal or meets the two triangles differently"""
    import test_tri_gpu as G
    from test_medium_gpu import _load
    out = []
    for cfg in G.tiling_cfgs():
        sc, c1, lens = _load(host, cfg, G.W, G.H, G.SPP, 8, seed=77)
        rc, rgb, lin, segs = lanes.render(sc.ptr, c1, sc.quads())
        rc2, rec = lanes.surface(sc.ptr, c1, sc.quads())
        assert rc == 0 and rc2 == 0
        out.append((rgb, lin, segs, rec, sc.c.n_spheres))
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]
    assert np.array_equal(_bits(a[3]["t"]), _bits(b[3]["t"]))
    n = a[4]
    on_floor = a[3]["id"] == n
    assert on_floor.sum() > 200 and set(np.unique(b[3]["id"][on_floor]).tolist()) == {n, n + 1}, "both triangles show, where the parallelogram showed"


def test_old_scenes_have_no_triangle(host):
    for path in ("scenes/cornell_spheres_600x600_spp128.json",):
        q = host.Scene.load(os.path.join(ROOT, path)).quads()
        assert len(q) == 17 and not any(x.reserved for x in q)
