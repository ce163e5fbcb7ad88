"""The ray tables of the structure's bit tests, shared by the host build's test (tests/test_flat_bvh_cpu.py) and the device's
(tests/test_flat_bvh_gpu.py).  A table is (quvs n x 9, shapes n, rays m x 6, closest m): ONE list of entries and rays that each meet the
whole list, where tests/quad_rays.py and tests/tri_rays.py pair every ray with one entry.

gathered(cls, lanes): a class of tests/tri_rays.py with its entries gathered into one list of at least 100 triangles (a class
with fewer than 100 entries is filled up with generic parallelograms behind them) and all its rays.
The classes aimed at the structure, 10^5 rays each (NEW_CLASSES):
  box_faces        rays through the vertices and along the edges of triangles: the points that lie exactly on the faces of their boxes
  zero_components  one or two direction components +0.0 / -0.0, a third of them with the origin in a face plane of a padded box (the slab
                   test's planes are grown by the ray's slack, so these do NOT reach the 0 * inf NaN: test_flat_bvh_cpu.py has the rays that do)
  flat_walls       axis-aligned walls, whose boxes have no thickness before the pad; rays in and beside their planes
  inside_boxes     origins inside padded boxes and exactly on their faces
  closest_ulps     closest_in within 3 ulps of an entry's t, on both sides and equal
  far_origins      a cluster of small entries and origins far away: |o| up to the precondition's limit 2^40 and one step beyond it"""
import numpy as np

from quad_rays import N_R, T_MAX, _aimed, _quads, _ulps
from tri_rays import tri_device_class_tables

NEW_CLASSES = ["box_faces", "zero_components", "flat_walls", "inside_boxes", "closest_ulps", "far_origins"]
OUTER = ("magnitudes", "non_finite")          # the classes of tri_rays.py that must reach the fallback
TRI, PAR = 1, 0


def gathered(cls, lanes):
    quvs, rays, closest = [], [], []
    for quv, r, c in tri_device_class_tables(cls, lanes):
        quvs.append(quv); rays.append(r); closest.append(c)
    shapes = [TRI] * len(quvs)
    if len(quvs) < 100:
        fill = _quads(np.random.default_rng(2200), 100)
        quvs += list(fill); shapes += [PAR] * len(fill)
    return np.array(quvs), np.array(shapes, np.uint32), np.concatenate(rays), np.concatenate(closest)


def _walls(rng, n):
    """axis-aligned parallelograms: u and v along two axes, either sign"""
    q = rng.uniform(-8.0, 8.0, (n, 3))
    quv = np.zeros((n, 9))
    quv[:, :3] = q
    for k in range(n):
        a, b = rng.permutation(3)[:2]
        quv[k, 3 + a] = rng.uniform(0.5, 6.0) * rng.choice([-1.0, 1.0])
        quv[k, 6 + b] = rng.uniform(0.5, 6.0) * rng.choice([-1.0, 1.0])
    return quv


def _closest(rng, n):
    return np.where(rng.random(n) < 0.5, T_MAX, rng.uniform(0.0, 12.0, n))


def _box_faces(sim, abi):
    rng = np.random.default_rng(2301)
    quvs = np.concatenate([_quads(rng, 60), _walls(rng, 40)])
    shapes = np.full(100, TRI, np.uint32)
    rays = []
    for quv in quvs:
        ab = rng.uniform(0.0, 1.0, (N_R, 2))
        kind = rng.integers(0, 4, N_R)
        ab[kind == 0] = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])[rng.integers(0, 3, int((kind == 0).sum()))]      # a vertex, exactly
        ab[kind == 1, 1] = 0.0                                                                                         # the edge b = 0
        ab[kind == 2, 0] = 0.0                                                                                         # the edge a = 0
        ab[kind == 3, 1] = 1.0 - ab[kind == 3, 0]                                                                      # the hypotenuse
        ab = np.where((rng.random((N_R, 2)) < 0.3) & (ab > 0.0), _ulps(ab + 0.0, rng.integers(-3, 4, (N_R, 2))), ab)      # (an ulp beside: only off 0)
        r = _aimed(rng, quv, N_R, ab)
        # a tenth start at the origin itself, where the ray's slack is zero: only the entry's own pad stands between the vertex and its box face
        zero_o = np.arange(N_R) % 10 == 0
        scale = rng.uniform(0.25, 4.0, (N_R, 1))
        r[zero_o] = np.concatenate([np.zeros((N_R, 3)), (quv[0:3] + ab[:, :1] * quv[3:6] + ab[:, 1:] * quv[6:9]) * scale], axis=1)[zero_o]
        rays.append(r)
    rays = np.concatenate(rays)
    return quvs, shapes, rays, _closest(rng, len(rays))


def _zero_components(sim, abi):
    import flat_bvh_sim as F
    rng = np.random.default_rng(2302)
    quvs = np.concatenate([_walls(rng, 50), _quads(rng, 50)])
    shapes = rng.integers(0, 2, 100).astype(np.uint32)
    ok, lo, hi = sim.entry_boxes(F.flats_array(abi, quvs, shapes))
    assert ok.all()
    rays = []
    for k, quv in enumerate(quvs):
        r = _aimed(rng, quv, N_R)
        zero = rng.random((N_R, 3)) < 0.45
        zero[zero.all(axis=1), 0] = False                            # one or two components, never all three
        zero[~zero.any(axis=1), rng.integers(0, 3)] = True
        r[:, 3:] = np.where(zero, np.where(rng.random((N_R, 3)) < 0.5, 0.0, -0.0), r[:, 3:])
        # a third of them start in a face plane of this entry's padded box: the origin's zeroed coordinate is lo or hi itself
        for i in range(0, N_R, 3):
            ax = int(np.flatnonzero(zero[i])[0])
            r[i, ax] = (lo if rng.random() < 0.5 else hi)[k, ax]
        rays.append(r)
    rays = np.concatenate(rays)
    return quvs, shapes, rays, _closest(rng, len(rays))


def _flat_walls(sim, abi):
    rng = np.random.default_rng(2303)
    quvs = _walls(rng, 100)
    shapes = rng.integers(0, 2, 100).astype(np.uint32)
    rays = []
    for quv in quvs:
        r = _aimed(rng, quv, N_R)
        n_ax = int(np.flatnonzero((quv[3:6] == 0.0) & (quv[6:9] == 0.0))[0])     # the wall's normal axis
        graze = rng.random(N_R) < 0.3
        r[graze, 3 + n_ax] *= 10.0 ** rng.uniform(-12, -2, int(graze.sum()))      # nearly in the plane
        onp = rng.random(N_R) < 0.1
        r[onp, n_ax] = quv[n_ax]                                                  # the origin in the wall's plane
        rays.append(r)
    rays = np.concatenate(rays)
    return quvs, shapes, rays, _closest(rng, len(rays))


def _inside_boxes(sim, abi):
    import flat_bvh_sim as F
    rng = np.random.default_rng(2304)
    quvs = np.concatenate([_quads(rng, 70), _walls(rng, 30)])
    shapes = rng.integers(0, 2, 100).astype(np.uint32)
    ok, lo, hi = sim.entry_boxes(F.flats_array(abi, quvs, shapes))
    assert ok.all()
    rays = []
    for k in range(100):
        o = lo[k] + rng.random((N_R, 3)) * (hi[k] - lo[k])
        face = rng.random((N_R, 3)) < 0.25
        o = np.where(face, np.where(rng.random((N_R, 3)) < 0.5, lo[k], hi[k]), o)
        rays.append(np.concatenate([o, rng.standard_normal((N_R, 3)) * rng.uniform(0.25, 4.0, (N_R, 1))], axis=1))
    rays = np.concatenate(rays)
    return quvs, shapes, rays, _closest(rng, len(rays))


def _closest_ulps(sim, abi):
    import flat_bvh_sim as F
    rng = np.random.default_rng(2305)
    quvs = np.concatenate([_quads(rng, 80), _walls(rng, 20)])
    shapes = rng.integers(0, 2, 100).astype(np.uint32)
    rays = np.concatenate([_aimed(rng, q, N_R, rng.uniform(0.05, 0.6, (N_R, 2)) * [1.0, 0.7]) for q in quvs])
    best, t, _ = sim.hit(F.flats_array(abi, quvs, shapes), rays, np.full(len(rays), T_MAX), False)
    assert (best >= 0).mean() > 0.9
    closest = np.where(best >= 0, _ulps(np.where(best >= 0, t, 1.0), rng.integers(-3, 4, len(rays))), T_MAX)
    return quvs, shapes, rays, closest


def _far_origins(sim, abi):
    rng = np.random.default_rng(2306)
    quvs = _quads(rng, 100) * 0.001           # a cluster of SMALL entries (a few thousandths across, within 0.01 of the origin): tight boxes, tiny pads
    shapes = rng.integers(0, 2, 100).astype(np.uint32)
    n = 100 * N_R
    which = np.repeat(np.arange(100), N_R)
    ab = rng.uniform(-0.2, 1.2, (n, 2))
    target = quvs[which, 0:3] + ab[:, :1] * quvs[which, 3:6] + ab[:, 1:] * quvs[which, 6:9]
    dirs = rng.standard_normal((n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dist = 2.0 ** rng.uniform(0.0, 40.5, (n, 1))
    o = target - dirs * dist
    # a tenth: one coordinate exactly the limit 2^40, and one step beyond it (which must take the fallback)
    edge = np.arange(n) % 10 == 0
    ax = rng.integers(0, 3, n)
    lim = np.where(np.arange(n) % 20 == 0, np.nextafter(2.0 ** 40, np.inf), 2.0 ** 40) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
    o[edge, ax[edge]] = lim[edge]
    d = (target - o) * rng.uniform(0.25, 4.0, (n, 1))
    return quvs, shapes, np.concatenate([o, d], axis=1), np.full(n, T_MAX)


_NEW = {"box_faces": _box_faces, "zero_components": _zero_components, "flat_walls": _flat_walls, "inside_boxes": _inside_boxes,
        "closest_ulps": _closest_ulps, "far_origins": _far_origins}


def new_class(cls, sim, abi):
    """(quvs, shapes, rays, closest) of one of NEW_CLASSES; sim: flat_bvh_sim.load(abi) (some classes read the padded boxes, one the scan's t)"""
    return _NEW[cls](sim, abi)
