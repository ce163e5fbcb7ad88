"""The structure over the flat primitives without a GPU: the host build of the builder, the traversal and the order-free
acceptance rule (tests/flatbvh/, bound by tests/flat_bvh_sim.py) against the host build of the full scan, bit for bit; the scene file's
key; the CPU build of the QUADS lane code with the structure bound."""
import importlib.util
import json
import os

import numpy as np
import pytest

import flat_bvh_rays as R
import flat_bvh_sim as F
import lane_sim
from quad_rays import T_MAX, _aimed, _quads
from tri_rays import TRI_CLASSES, tri_class_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_SHA256 = "bf3ccfcd7a095d77ca02d8c3afda75747b7845ca36bdca52a4b3931a080b93d4"   # of scenes/make_bvh_scene.py's output (175 KB: not committed)
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def sim(abi):
    return F.load(abi)


@pytest.fixture(scope="module")
def lanes(abi):
    return lane_sim.load(abi)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------ 1. build invariants
def heightfield(n=32, size=8.0, seed=5):
    """an n x n grid of cells, two triangles each (2 n^2 entries), heights from a fixed seed: quv rows"""
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.0, 0.6, (n + 1, n + 1))
    x = np.linspace(-size / 2, size / 2, n + 1)
    P = lambda i, j: np.array([x[i], h[i, j], x[j]])
    out = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1)
            out.append(np.concatenate([a, c - a, b - a]))     # wound so that N points up
            out.append(np.concatenate([a, d - a, c - a]))
    return np.array(out)


def _world(kind, n):
    """quv rows and shapes of one of the builder's worlds"""
    rng = np.random.default_rng(1000 + n)
    if kind == "generic":
        return _quads(rng, n), rng.integers(0, 2, n)
    if kind == "coplanar":        # every entry in the plane y = 1
        q = rng.uniform(-8, 8, (n, 3)); q[:, 1] = 1.0
        u = np.zeros((n, 3)); v = np.zeros((n, 3))
        u[:, 0] = rng.uniform(0.1, 2, n); v[:, 2] = rng.uniform(0.1, 2, n)
        return np.concatenate([q, u, v], axis=1), rng.integers(0, 2, n)
    if kind == "identical":
        return np.tile([[0.5, -1.0, 2.0, 1.5, 0.0, 0.25, 0.0, 2.0, 0.5]], (n, 1)), np.zeros(n, int)
    if kind == "wall_and_small":  # one huge wall first, the rest small
        quv = _quads(rng, n) * ([1.0] * 3 + [0.05] * 6)
        quv[0] = [-500.0, -1.0, -500.0, 1000.0, 0.0, 0.0, 0.0, 0.0, 1000.0]
        return quv, np.concatenate([[0], rng.integers(0, 2, n - 1)])
    if kind == "outliers":        # every fifth entry outside the preconditions: a needle, a sliver, a far one
        quv = _quads(rng, n)
        for k in range(0, n, 5):
            quv[k] = [[0, 0, 0, 1e9, 0, 0, 0, 1e-3, 0], [0, 0, 0, 1, 0, 0, 1, 1e-9, 0], [3e12, 0, 0, 1, 0, 0, 0, 1, 0]][(k // 5) % 3]
        return quv, rng.integers(0, 2, n)
    raise KeyError(kind)


WORLDS = [(k, n) for n in (1, 4, 5, 9, 33, 1024, 1025, 4096) for k in ("generic",)] + [("coplanar", 33), ("coplanar", 1025), ("identical", 5),
          ("identical", 1025), ("wall_and_small", 9), ("wall_and_small", 4096), ("outliers", 33), ("outliers", 1025)]


@pytest.mark.parametrize("kind,n", WORLDS)
def test_build_invariants(sim, abi, kind, n):
    """every entry in exactly one leaf; every leaf entry's padded box inside all its ancestors' boxes; skip strictly increasing along any
    walk; two builds give the same bytes; the entries outside the preconditions sit in the always-visited run.  Exact comparisons only."""
    quv, shapes = _world(kind, n)
    flats = F.flats_array(abi, quv, shapes)
    nodes, order, n_always = sim.build(flats)
    again = sim.build(flats)
    assert nodes.tobytes() == again[0].tobytes() and order.tobytes() == again[1].tobytes() and n_always == again[2]
    assert sorted(order.tolist()) == list(range(n))
    ok, lo, hi = sim.entry_boxes(flats)
    assert n_always == int((~ok).sum()) and (n_always > 0) == (kind == "outliers")
    nn = len(nodes)
    assert sim.check(nodes, order, n) == ""
    skip, first, count = nodes["skip"].astype(np.int64), nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    assert (skip > np.arange(nn)).all() and (skip <= nn).all() and (count <= 4).all() and (first + count <= n).all()
    # the always-visited run: the first ceil(n_always / 4) nodes, infinite boxes, the refused entries in entry order
    n_run = (n_always + 3) // 4
    run = nodes[:n_run]
    assert np.isneginf(run["lo"]).all() and np.isposinf(run["hi"]).all() and (run["count"] > 0).all() and (run["skip"] == np.arange(1, n_run + 1)).all()
    assert order[:n_always].tolist() == np.flatnonzero(~ok).tolist()
    assert np.isfinite(nodes[n_run:]["lo"]).all() and np.isfinite(nodes[n_run:]["hi"]).all()
    # the leaves partition the order table, in order; a leaf's entries are in index order
    leaves = np.flatnonzero(count > 0)
    assert first[leaves].tolist() == np.concatenate([[0], np.cumsum(count[leaves])[:-1]]).tolist() and int(count[leaves].sum()) == n
    # walk the tree with a stack of (node, end of its subtree): children lie inside, skips are the subtree ends
    seen = np.zeros(n, int)
    for r in range(n_run):
        seen[order[first[r]:first[r] + count[r]]] += 1
    stack = [(n_run, nn, np.full(3, -np.inf), np.full(3, np.inf))] if n_run < nn else []
    while stack:
        i, end, plo, phi = stack.pop()
        nd = nodes[i]
        assert skip[i] == end and (nd["lo"] >= plo).all() and (nd["hi"] <= phi).all()
        if count[i]:
            ks = order[first[i]:first[i] + count[i]]
            assert ks.tolist() == sorted(ks.tolist()) and end == i + 1
            seen[ks] += 1
            assert (lo[ks] >= nd["lo"]).all() and (hi[ks] <= nd["hi"]).all() and ok[ks].all()
            assert (nd["lo"] == lo[ks].min(axis=0)).all() and (nd["hi"] == hi[ks].max(axis=0)).all()
        else:
            left = i + 1
            right = int(skip[left])
            assert i < left < right < end
            stack.append((left, right, nd["lo"], nd["hi"]))
            stack.append((right, end, nd["lo"], nd["hi"]))
    assert (seen == 1).all()
    if n > 4 and n_always == 0:
        assert count[0] == 0, "more than four entries: an inner node"


def test_pads_are_positive_and_boxes_hold_their_corners(sim, abi):
    """a zero-thickness wall has a box of positive thickness; every corner of an entry lies strictly inside its padded box"""
    quv = np.concatenate([R._walls(np.random.default_rng(3), 50), _quads(np.random.default_rng(4), 50)])
    shapes = np.arange(100) % 2
    ok, lo, hi = sim.entry_boxes(F.flats_array(abi, quv, shapes))
    assert ok.all() and (hi > lo).all()
    for k in range(100):
        q, u, v = quv[k, :3], quv[k, 3:6], quv[k, 6:]
        for c in [q, q + u, q + v] + ([q + u + v] if shapes[k] == 0 else []):
            assert (lo[k] < c).all() and (c < hi[k]).all()


def test_build_time_checks_refuse_bad_tables(sim, abi):
    quv, shapes = _world("generic", 33)
    nodes, order, _ = sim.build(F.flats_array(abi, quv, shapes))
    assert sim.check(nodes, order, 33) == ""
    for field, at, value, msg in (("skip", 0, 0, "skip"), ("skip", 3, 3, "skip"), ("skip", 1, len(nodes) + 1, "skip"), ("first", len(nodes) - 1, 33, "leaf"),
                                  ("count", len(nodes) - 1, 5, "leaf")):
        bad = nodes.copy()
        bad[field][at] = value
        assert msg in sim.check(bad, order, 33), (field, at)
    dup = order.copy(); dup[1] = dup[0]
    assert "permutation" in sim.check(nodes, dup, 33)
    big = order.copy(); big[5] = 33
    assert "permutation" in sim.check(nodes, big, 33)
    assert "one entry per primitive" in sim.check(nodes, order[:-1], 33)


# ------------------------------------------------------------------ 2., 3. the structure equals the scan, bit for bit
def _equal(sim, abi, name, quvs, shapes, rays, closest, id_base=3):
    flats = F.flats_array(abi, quvs, shapes)
    with np.errstate(all="ignore"):
        b0, t0, _ = sim.hit(flats, rays, closest, False, id_base)
        b1, t1, cnt = sim.hit(flats, rays, closest, True, id_base)
        okay = F.ray_ok(rays)
    n, hits = len(rays), int((b0 >= 0).sum())
    print(f"{name}: {len(flats)} entries, {n} rays, {hits} hit; structure {cnt['rays_bvh']} scan {cnt['rays_scan']}; "
          f"per ray {cnt['entry_tests'] / max(1, cnt['rays_bvh']):.2f} entry tests, {cnt['box_tests'] / max(1, cnt['rays_bvh']):.2f} box tests")
    bad = np.flatnonzero((b0 != b1) | (_bits(t0) != _bits(t1)))
    assert bad.size == 0, f"{name}: {bad.size} rays differ; first {bad[:5].tolist()}: scan {b0[bad[:5]].tolist()} structure {b1[bad[:5]].tolist()}"
    assert cnt["rays_bvh"] == int(okay.sum()) and cnt["rays_scan"] == int((~okay).sum())
    return b0, cnt, okay


@pytest.mark.parametrize("cls", TRI_CLASSES)
def test_classes_of_the_flat_primitive_tests_gathered_into_one_list(sim, lanes, abi, cls):
    """the ten ray classes of tests/tri_rays.py, their entries gathered into one list of >= 100: (best, bits of t) of the structure equal the
    scan's.  `magnitudes` and `non_finite` reach the fallback — exactly the rays flat_ray_ok refuses, counted — and are equal all the
    same; every ray of the other classes takes the structure."""
    quvs, shapes, rays, closest = R.gathered(cls, lanes)
    assert len(quvs) >= 100 and len(rays) >= 100_000
    b0, cnt, okay = _equal(sim, abi, cls, quvs, shapes, rays, closest)
    if cls in R.OUTER:
        assert cnt["rays_scan"] > 0.3 * len(rays), "the outer classes must reach the fallback"
        assert cnt["rays_bvh"] > 0
    else:
        # (only the rays with a non-finite component: `den` has 5 % whose d_z is 0 or subnormal and whose d_x, d_y are NaN or inf for it)
        finite = np.isfinite(rays).all(axis=1)
        assert np.array_equal(okay, finite) and cnt["rays_scan"] == int((~finite).sum()) <= 0.05 * len(rays) and (finite.all() or cls == "den")
    if cls not in ("magnitudes", "non_finite", "on_plane"):
        assert 0.02 * len(rays) < (b0 >= 0).sum() < 0.999 * len(rays)


@pytest.mark.parametrize("cls", R.NEW_CLASSES)
def test_classes_aimed_at_the_structure(sim, abi, cls):
    quvs, shapes, rays, closest = R.new_class(cls, sim, abi)
    assert len(rays) >= 100_000 and len(quvs) >= 100
    b0, cnt, okay = _equal(sim, abi, cls, quvs, shapes, rays, closest)
    assert 0.02 * len(rays) < (b0 >= 0).sum()
    if cls == "far_origins":      # the limit itself is inside, one step beyond it is outside
        beyond = (np.abs(rays[:, :3]) > F.RAY_O_MAX).any(axis=1)
        at = (np.abs(rays[:, :3]) == F.RAY_O_MAX).any(axis=1) & ~beyond
        assert beyond.sum() >= 4000 and at.sum() >= 4000 and okay[at].all() and not okay[beyond].any()
        assert cnt["rays_scan"] == int((~okay).sum()) > 0
    else:
        assert cnt["rays_scan"] == 0
    if cls == "zero_components":
        z = (rays[:, 3:] == 0.0).sum(axis=1)
        assert ((z == 1) | (z == 2)).all() and (z == 2).sum() > 1000 and np.signbit(rays[:, 3:][rays[:, 3:] == 0.0]).sum() > 1000
    if cls == "closest_ulps":     # both sides and equal: the scan's own answer differs between them
        assert 0.2 * len(rays) < (b0 >= 0).sum() < 0.9 * len(rays)


def test_a_slab_axis_that_meets_a_nan_visits(sim, abi):
    """rays with d_k = +-0.0 whose origin lies EXACTLY in a grown face plane of the root's box, o_k = fl(lo_k - s(o)) or fl(hi_k + s(o)) found
    by fixed-point iteration (s depends on o_k): (lo_k - s) - o_k is 0, times 1 / d_k = inf a NaN.  The counters show that the NaN arises
    and that the root is visited all the same (its children are tested); the result is the scan's."""
    quv, shapes = _world("generic", 33)
    flats = F.flats_array(abi, quv, shapes)
    nodes, _, _ = sim.build(flats)
    lo, hi = nodes["lo"][0], nodes["hi"][0]
    rng = np.random.default_rng(404)
    rays = []
    for i in range(3000):
        ax, low = i % 3, (i // 3) % 2 == 0
        o = lo + rng.random(3) * (hi - lo)
        d = rng.standard_normal(3)
        d[ax] = 0.0 if i % 4 < 2 else -0.0
        slack = lambda: 2.0 ** -30 * ((abs(o[0]) + abs(o[1])) + abs(o[2]))       # rt_core.h: s, in its operation order
        for _ in range(6):
            o[ax] = lo[ax] - slack() if low else hi[ax] + slack()
        if ((lo[ax] - slack()) - o[ax] if low else (hi[ax] + slack()) - o[ax]) == 0.0:
            rays.append(np.concatenate([o, d]))
    rays = np.array(rays)
    assert len(rays) >= 2000
    far = np.full(len(rays), T_MAX)
    b0, t0, _ = sim.hit(flats, rays, far, False)
    b1, t1, cnt = sim.hit(flats, rays, far, True)
    assert np.array_equal(b0, b1) and np.array_equal(_bits(t0), _bits(t1)) and cnt["rays_scan"] == 0
    assert cnt["nan_axes"] >= len(rays), "every ray meets the NaN at the root"
    assert cnt["box_tests"] >= 3 * len(rays), "... and the root is visited: both its children are tested"


# ------------------------------------------------------------------ 4. ties
def _tie_world(swap=False):
    """eight parallelograms spread along z, so that the root splits them four and four by the z of their centres.  A and B lie in ONE plane
    (x = 0: N = (1, 0, 0), D = 0, so both give a ray the same t in every bit) and overlap on 0 <= z <= 2; B's centre (z = 0) sorts into the
    left leaf, A's (z = 2) into the right one.  A is entry 1 and B entry 6 — the LARGER index is visited first — or, swapped, B is 1 and A 6."""
    quv = np.zeros((8, 9))
    for k, z in zip((0, 2, 3, 4, 5, 7), (-20.0, -15.0, -10.0, 10.0, 15.0, 20.0)):
        quv[k] = [0.5, -0.25, z, 0.0, 0.5, 0.0, 0.0, 0.0, 0.5]
    A, B = [0.0, -1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 4.0], [0.0, -1.0, -2.0, 0.0, 2.0, 0.0, 0.0, 0.0, 4.0]
    quv[1], quv[6] = (B, A) if swap else (A, B)
    return quv, np.zeros(8, int)


def _tie_rays(n=4000):
    """from x = -9 into the overlap of A and B"""
    rng = np.random.default_rng(78)
    target = np.stack([np.zeros(n), rng.uniform(-0.9, 0.9, n), rng.uniform(0.1, 1.9, n)], axis=1)
    o = np.tile([-9.0, 0.0, 0.0], (n, 1))
    return np.concatenate([o, target - o], axis=1)


@pytest.mark.parametrize("swap", [False, True])
def test_coincident_entries_in_different_leaves_the_smaller_index_wins(sim, abi, swap):
    quv, shapes = _tie_world(swap)
    flats = F.flats_array(abi, quv, shapes)
    nodes, order, _ = sim.build(flats)
    # the placement, from the tables: a root, two leaves of four; entries 1 and 6 in different leaves, the one with its centre at z = 0 first
    assert nodes["count"].tolist() == [0, 4, 4] and nodes["skip"].tolist() == [3, 2, 3]
    left, right = order[:4].tolist(), order[4:].tolist()
    assert (left, right) == (([0, 1, 2, 3], [4, 5, 6, 7]) if swap else ([0, 2, 3, 6], [1, 4, 5, 7]))
    rays = _tie_rays()
    far = np.full(len(rays), T_MAX)
    b0, t0, _ = sim.hit(flats, rays, far, False, 2)
    b1, t1, cnt = sim.hit(flats, rays, far, True, 2)
    assert (b0 == 2 + 1).all() and np.array_equal(b0, b1) and np.array_equal(_bits(t0), _bits(t1)) and cnt["rays_scan"] == 0
    assert cnt["entry_tests"] == 8 * len(rays), "both leaves are visited: the two entries are met in node order"
    # the two really tie: each alone gives the same t in every bit
    for k in (1, 6):
        bk, tk, _ = sim.hit(F.flats_array(abi, quv[[k]], [0]), rays, far, True, 2 + k)
        assert (bk == 2 + k).all() and np.array_equal(_bits(tk), _bits(t1))
    # a sphere at the exact tie still wins, and tie_ok is never applied against a sphere: closest_in = the entries' own t, best_in = a sphere
    for sphere in (0, 1):
        held = np.full(len(rays), sphere, np.int32)
        bs, ts, _ = sim.hit(flats, rays, t1, True, 2, held)
        b_scan, t_scan, _ = sim.hit(flats, rays, t1, False, 2, held)
        assert (bs == sphere).all() and np.array_equal(_bits(ts), _bits(t1)) and np.array_equal(bs, b_scan) and np.array_equal(_bits(ts), _bits(t_scan))


# ------------------------------------------------------------------ 5. work is cut
def test_work_is_cut_on_a_heightfield(sim, abi):
    """a 32 x 32 heightfield of 2 048 triangles under 10^4 downward camera-like rays: the mean number of entry tests per ray through the
    structure is at most 1 / 8 of the entry count (measured on the host build: 4.69 entry tests and 15.45 box tests per ray)"""
    quv = heightfield()
    assert len(quv) == 2048
    rng = np.random.default_rng(9)
    o = np.tile([0.0, 9.0, 0.5], (10_000, 1))
    target = np.stack([rng.uniform(-5, 5, 10_000), np.zeros(10_000), rng.uniform(-5, 5, 10_000)], axis=1)
    rays = np.concatenate([o, target - o], axis=1)
    b0, cnt, _ = _equal(sim, abi, "heightfield", quv, np.ones(2048, int), rays, np.full(10_000, T_MAX), id_base=0)
    assert (b0 >= 0).mean() > 0.5
    assert cnt["entry_tests"] / cnt["rays_bvh"] <= 2048 / 8


# ------------------------------------------------------------------ 6. rt_flat_hit_tie
@pytest.mark.parametrize("cls", TRI_CLASSES)
def test_flat_hit_tie_without_the_tie_is_flat_hit(sim, cls):
    """decision and every output bit, on all ten class tables, for both limits"""
    n = 0
    for quv, rays, closest in tri_class_tables(cls):
        for lim in (1.0, 2.0):
            st, a, b = sim.tie(quv, lim, rays, closest, 0)
            if st:
                assert cls == "magnitudes"
                continue
            assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
            n += len(rays)
    assert n >= 100_000


def test_flat_hit_tie_accepts_exactly_the_equal_t(sim):
    from quad_rays import AXIS_QUV
    rng = np.random.default_rng(12)
    rays = _aimed(rng, AXIS_QUV, 5000, rng.uniform(0.1, 0.9, (5000, 2)))
    st, a, _ = sim.tie(AXIS_QUV, 2.0, rays, np.full(5000, T_MAX), 0)
    assert st == 0 and a[0].all()
    t = a[1]
    for k, want_plain, want_tie in ((0, 0, 1), (1, 1, 1), (-1, 0, 0)):
        closest = np.nextafter(t, np.inf) if k > 0 else (np.nextafter(t, -np.inf) if k < 0 else t)
        st, a2, b2 = sim.tie(AXIS_QUV, 2.0, rays, closest, 1)
        assert (a2[0] == want_plain).all() and (b2[0] == want_tie).all()
        assert np.array_equal(_bits(b2[1][b2[0] == 1]), _bits(t[b2[0] == 1]))


# ------------------------------------------------------------------ 7. schema
def _file(n_faces, key=None):
    verts = [[0.1, 0.0, 0.3], [1.7, 0.2, 0.0], [0.3, 1.9, 0.1]]
    cfg = {"width": 8, "height": 8, "samples_per_pixel": 1, "max_depth": 2, "sky": {"texture": ""},
           "camera": {"look_from": {"x": 0.0, "y": 1.0, "z": 5.0}, "look_at": {"x": 0.0, "y": 0.0, "z": 0.0}, "vup": {"x": 0.0, "y": 1.0, "z": 0.0}, "vfov": 40.0,
                      "aspect": 1.0},
           "objects": [{"center": {"x": 0.0, "y": 1.0, "z": 0.0}, "radius": 0.5, "material": {"Glass": {"index_of_refraction": 1.5}}},
                       {"mesh": {"vertices": verts, "faces": [[0, 1, 2]] * n_faces}, "material": {"Lambertian": {"albedo": [0.5, 0.25, 0.75]}}}]}
    if key is not None:
        cfg["flat_bvh"] = key
    return json.dumps(cfg, separators=(",", ":"))


def test_the_key_and_its_round_trip(host, abi):
    for key, want in ((None, False), (False, False), (True, True)):
        sc = host.Scene.loads(_file(3, key))
        assert sc.flat_bvh() is want and len(sc.quads()) == 3
        text = sc.to_json()
        assert text.count('"flat_bvh":true') == (1 if want else 0) and text.count("flat_bvh") == (1 if want else 0)
        again = host.Scene.loads(text)
        assert again.flat_bvh() is want and again.to_json() == text
    for bad in (1, "true", [True]):
        with pytest.raises(host.RtError) as e:
            host.Scene.loads(_file(3, bad))
        assert e.value.code == abi.RT_ERR_PARSE and "flat_bvh" in str(e.value)
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_file(3).replace('"objects"', '"flat_bvh":null,"objects"'))
    assert "flat_bvh" in str(e.value)


def test_1025_triangles_load_with_the_key_and_are_refused_without(host, abi):
    ok = host.Scene.loads(_file(1025, True))
    assert len(ok.quads()) == 1025 and ok.flat_bvh()
    for key in (None, False):
        with pytest.raises(host.RtError) as e:
            host.Scene.loads(_file(1025, key))
        assert e.value.code == abi.RT_ERR_UNSUPPORTED and "objects[1]" in str(e.value) and "1024" in str(e.value), str(e.value)
    # load errors still name their object with the key
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_file(5, True).replace("[0,1,2]]", "[0,1,7]]"))
    assert "objects[1]" in str(e.value)


def test_the_example_equals_its_generators_output(host, abi):
    spec = importlib.util.spec_from_file_location("make_bvh_scene", os.path.join(ROOT, "scenes", "make_bvh_scene.py"))
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scenes"))
    try:
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scenes"))
    import hashlib
    text = mod.make()
    assert hashlib.sha256(text.encode()).hexdigest() == EXAMPLE_SHA256 and len(text) < 512 * 1024
    sc = host.Scene.loads(text)
    q = sc.quads()
    assert sc.flat_bvh() and len(q) == 5 + 5120 + 1280 and sum(x.reserved for x in q) == 6400
    assert [x.kind for x in q[5:5125]] == [abi.RT_MAT_GLASS] * 5120 and [x.kind for x in q[5125:]] == [abi.RT_MAT_METAL] * 1280
    # wound outward: every N points away from its sphere's centre
    for lo, hi, centre in ((5, 5125, (390.0, 110.0, 170.0)), (5125, 6405, (190.0, 125.0, 380.0))):
        quv = np.array([list(x.q) + list(x.u) + list(x.v) for x in q[lo:hi]])
        nrm = np.cross(quv[:, 3:6], quv[:, 6:9])
        mid = quv[:, :3] + (quv[:, 3:6] + quv[:, 6:9]) / 3.0 - np.array(centre)
        assert ((nrm * mid).sum(axis=1) > 0).all()
    big = json.loads(mod.make(5))
    assert len(big["objects"][-1]["mesh"]["faces"]) == 20 * 4 ** 5 and big["flat_bvh"] is True


# ------------------------------------------------------------------ 8. the lane code with the structure bound
def test_lane_code_with_the_structure_equals_the_scan(sim, host, abi):
    """the CPU build of the QUADS lane code on the pinhole parity frames of tests/test_flat_bvh_gpu.py: linear radiance, RGB8 and segments"""
    import test_flat_bvh_gpu as G
    for case, depth in G.FRAME_CASES:
        if "lens" in case:
            continue
        sc, c1, lens, quads = G.frame_world(host, case, depth)
        rc0, rgb0, lin0, segs0, cnt0 = sim.render(sc.ptr, False, c1, quads)
        rc1, rgb1, lin1, segs1, cnt1 = sim.render(sc.ptr, True, c1, quads)
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(rgb0, rgb1) and np.array_equal(lin0.view(np.uint32), lin1.view(np.uint32)) and segs0 == segs1, case
        assert cnt0["rays_bvh"] == cnt0["rays_scan"] == 0 and cnt1["rays_bvh"] + cnt1["rays_scan"] >= segs1 > 0, case
        assert len(np.unique(rgb1.reshape(-1, 3), axis=0)) > 50
