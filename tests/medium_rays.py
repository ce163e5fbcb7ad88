"""The ray tables of the media code's bit tests, shared by the host build's test (tests/test_medium_cpu.py) and the device's
(tests/test_medium_rays_gpu.py): eight classes of (world, rays, nodes), N_W worlds x N_R rays each, every class aimed at one decision of
rt_core.h medium_hit; and the seven adversarial walk worlds of tests/test_medium_cpu.py with their ray tables.

A world is a list of objects (centre, radius, "medium" | "opaque", density), built through the C structs by scene(); ray i of a world has
the RNG address (pixel i, sample 0, node nodes[i], the world's seed).  class_worlds(cls, L) draws a class once per session from a fixed
seed (L = tests/lane_sim.py's simulator: boundary_density asks the host build for each ray's draw and chord before it sets the
densities); class_reference(cls, abi, L) is the host build's answer — hit_world_v's (best, t, work) and medium_terms_v's figures for the
sphere each ray is aimed at — which the tests without the gpu mark state the classes' conditions on and the device tests compare with.

  generic           origins outside and inside one or two media, density 10^U(-2, 2)
  tangent           impact parameter r (1 + j 2^-52), j = -8 .. 8, and r (1 +- 10^U(-15, -6)); axis-parallel rays past whole-number spheres
                    (discriminant exactly 0); spheres of radius ~2^-520, whose discriminants lie in the denormal range
  surface_origin    small spheres near the origin, where an ulp of a coordinate is an ulp of T_MIN: origins placed so that t1 or t2 comes
                    out at T_MIN (1 + k 2^-52), k = -4 .. 4, and chords shorter than T_MIN
  boundary_density  1 000 media per world, ray i through medium i, whose density is set from the host build's u and chord so that the
                    free-flight distance is the chord times (1 + j 2^-52), j = -2 .. 2
  magnitudes        |d| from 1e-150 to 1e150 (beyond [1e-75, 1e75] ray_consts takes its slow path), centres up to 1e6, radii 1e-3 .. 1e4,
                    density 1e-12 .. 1e12
  occluder_inside   an opaque sphere inside the medium, on the ray; the density puts the candidate before it about half the time
  nested            two concentric media of different radius and density, in either table order
  non_finite        generic worlds; NaN, +-inf and +-1e308 components in origin or direction (through the probe only, never a frame)"""
import ctypes as C

import numpy as np

import adversarial_rays as AR

CLASSES = ["generic", "tangent", "surface_origin", "boundary_density", "magnitudes", "occluder_inside", "nested", "non_finite"]
FRAME_CLASSES = ("generic", "tangent", "surface_origin", "boundary_density", "occluder_inside", "nested")   # finite rays of ordinary magnitude
N_W, N_R = 100, 1000          # 1 000 rays = 15 waves + 40 lanes: the last wave of a launch is partial
NODES = np.array([0, 1, 7, 0x80000002, 0xFFFFFFFE], np.uint32)
T_MIN = 0.001
EPS = 2.0 ** -52


class World:
    """objs = [(centre, radius, "medium" | "opaque", density)], rays (n x 6), nodes (n), target (n: the object each ray is aimed at), seed,
    and per-class notes (dict of arrays, e.g. the j of a boundary ray)"""

    def __init__(self, objs, rays, nodes, target, seed, **notes):
        self.objs, self.seed, self.notes = objs, seed, notes
        self.rays = np.ascontiguousarray(rays, np.float64)
        self.nodes = np.ascontiguousarray(nodes, np.uint32)
        self.target = np.ascontiguousarray(target, np.int64)
        for a in (self.rays, self.nodes, self.target):
            a.setflags(write=False)

    def is_medium(self):
        return np.array([o[2] == "medium" for o in self.objs])

    def spheres4(self):
        """n x 4 {centre, radius} of each ray's target"""
        g = np.array([[*o[0], o[1]] for o in self.objs], np.float64)
        return g[self.target]

    def densities(self):
        return np.array([o[3] for o in self.objs], np.float64)[self.target]


def scene(abi, objs, seed, width=8, height=8, spp=1, depth=2):
    """an RtScene over objs, gradient sky -> (scene, the array that keeps its spheres alive)"""
    arr = (abi.RtSphere * len(objs))()
    for s, (c, r, kind, dens) in zip(arr, objs):
        s.center[:] = [float(x) for x in c]
        s.radius = float(r)
        s.albedo[:] = [0.6, 0.5, 0.7]
        if kind == "medium":
            s.kind, s.fuzz_or_ior = abi.RT_MAT_MEDIUM, float(dens)
        else:
            s.kind = abi.RT_MAT_LAMBERTIAN
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=width, height=height, samples_per_pixel=spp, max_depth=depth, sky_mode=abi.RT_SKY_GRADIENT,
                     spheres=arr, n_spheres=len(objs), seed=seed)
    sc.cam_origin[:] = [0.0, 0.0, 30.0]               # (a probe frame's camera rays are the caller's; the camera is an ordinary one)
    sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]
    sc.cam_horizontal[:] = [3.0, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    return sc, arr


# ------------------------------------------------------------------ ray families
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _through(rng, c, r, n, spread=0.9, far=(1.2, 6.0)):
    """n rays from outside the ball (c, r) — c, r scalars or per ray — through a point within spread * r of its centre"""
    c, r = np.broadcast_to(np.asarray(c, np.float64), (n, 3)), np.broadcast_to(np.asarray(r, np.float64), (n,))
    o = c + _unit(rng, n) * (r * rng.uniform(*far, n))[:, None]
    aim = c + rng.uniform(-1.0, 1.0, (n, 3)) * (r * spread / np.sqrt(3.0))[:, None]
    return np.concatenate([o, (aim - o) * rng.uniform(0.2, 2.0, (n, 1))], axis=1)


def _inside(rng, c, r, n):
    """n rays that start inside the ball, short and long directions"""
    c, r = np.broadcast_to(np.asarray(c, np.float64), (n, 3)), np.broadcast_to(np.asarray(r, np.float64), (n,))
    o = c + _unit(rng, n) * (r * rng.uniform(0.0, 0.95, n))[:, None]
    return np.concatenate([o, rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-2.0, 2.0, (n, 1))], axis=1)


def _mixed_rays(rng, objs, media, n):
    """half through, half inside, each ray aimed at one of the media -> rays, target"""
    target = np.array(media)[rng.integers(0, len(media), n)]
    c = np.array([objs[j][0] for j in target], np.float64)
    r = np.array([objs[j][1] for j in target], np.float64)
    rays = np.where((np.arange(n) % 2 == 0)[:, None], _through(rng, c, r, n), _inside(rng, c, r, n))
    return rays, target


def _perp(rng, u):
    w = np.cross(u, rng.standard_normal(u.shape))
    return w / np.linalg.norm(w, axis=1)[:, None]


def _generic_objs(rng):
    c, r = rng.uniform(-5.0, 5.0, 3), rng.uniform(0.5, 3.0)
    objs = [(c, r, "medium", 10.0 ** rng.uniform(-2.0, 2.0))]
    if rng.random() < 0.5:
        objs.append((c + rng.uniform(-1.0, 1.0, 3) * r * 1.5, rng.uniform(0.5, 3.0), "medium", 10.0 ** rng.uniform(-2.0, 2.0)))
    return objs


def _generic(rng, w, L):
    objs = _generic_objs(rng)
    rays, target = _mixed_rays(rng, objs, list(range(len(objs))), N_R)
    return objs, rays, target, {}


def _tangent(rng, w, L):
    n = N_R
    dens = 10.0 ** rng.uniform(6.0, 14.0)
    if w % 4 == 1:      # exactly tangent, representable: axis-parallel rays past a whole-number sphere, (oc.d)^2 - |d|^2 (|oc|^2 - r^2) = 0
        ci, ri = rng.integers(-4, 5, 3).astype(np.float64), float(rng.integers(1, 4))
        ax = rng.integers(0, 3, n); bx = (ax + 1) % 3
        o = np.tile(ci, (n, 1))
        o[np.arange(n), bx] += ri
        o[np.arange(n), ax] -= rng.integers(2, 9, n)
        d = np.zeros((n, 3))
        d[np.arange(n), ax] = rng.choice([0.5, 1.0, 2.0, 4.0], n)
        nudge = rng.random(n) < 0.5          # half of them an ulp or two off the tangent, either way
        o[np.arange(n), bx] += np.where(nudge, ri * rng.integers(-2, 3, n) * EPS, 0.0)
        return [(ci, ri, "medium", dens)], np.concatenate([o, d], axis=1), np.zeros(n, np.int64), {}
    if w % 4 == 3:      # a sphere of radius ~2^-520 at the origin: r^2, |oc|^2 and the discriminant are denormal numbers
        r = float(2.0 ** -520 * rng.uniform(1.0, 2.0))
        ax = rng.integers(0, 3, n); bx = (ax + 1) % 3
        o, d = np.zeros((n, 3)), np.zeros((n, 3))
        o[np.arange(n), ax] = -r * rng.uniform(2.0, 8.0, n)
        o[np.arange(n), bx] = r * np.where(rng.random(n) < 0.5, 1.0 + rng.integers(-8, 9, n) * EPS, rng.uniform(0.0, 1.3, n))
        d[np.arange(n), ax] = rng.choice([0.5, 1.0, 2.0], n)
        return [(np.zeros(3), r, "medium", dens)], np.concatenate([o, d], axis=1), np.zeros(n, np.int64), {}
    c, r = rng.uniform(-5.0, 5.0, 3), rng.uniform(0.5, 3.0)
    nrm = _unit(rng, n)
    tdir = _perp(rng, nrm)
    delta = np.where(rng.random(n) < 0.5, rng.integers(-8, 9, n) * EPS, rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15.0, -6.0, n))
    p = c + nrm * (r * (1.0 + delta))[:, None]
    o = p - tdir * rng.uniform(0.5, 30.0, (n, 1))
    return [(c, r, "medium", dens)], np.concatenate([o, tdir * rng.uniform(0.1, 3.0, (n, 1))], axis=1), np.zeros(n, np.int64), {}


def _surface_origin(rng, w, L):
    n = N_R
    c, r = rng.uniform(-1.0, 1.0, 3) * 2.0 ** -6, float(2.0 ** -8 * rng.uniform(1.0, 2.0))
    u = _unit(rng, n)
    wdir = _perp(rng, u)
    s = rng.choice([0.5, 1.0, 2.0], n)
    d = u * s[:, None]
    fam = rng.choice(3, n, p=[0.5, 0.3, 0.2])          # t1 at T_MIN; t2 at T_MIN; a chord shorter than T_MIN
    h_short = rng.uniform(0.05, 0.45, n) * T_MIN * s
    b = np.where(fam == 2, np.sqrt(np.maximum(r * r - h_short * h_short, 0.0)), r * rng.uniform(0.0, 0.9, n))
    h = np.sqrt(r * r - b * b)
    mid = c + wdir * b[:, None]
    at = np.where((fam == 1)[:, None], mid + u * h[:, None], mid - u * h[:, None])      # the exit point, else the entry point
    k = rng.integers(-4, 5, n)
    back = np.where((fam == 2) & (rng.random(n) < 0.5), rng.uniform(0.0, 3.0, n) * T_MIN, T_MIN * (1.0 + k * EPS))
    o = at - d * back[:, None]
    return [(c, r, "medium", 10.0 ** rng.uniform(2.5, 5.0))], np.concatenate([o, d], axis=1), np.zeros(n, np.int64), {"fam": fam}


def _boundary_density(rng, w, L, seed, nodes):
    """N_R media on a jittered lattice, ray i through medium i; the densities from the host build's figures"""
    n = N_R
    g = np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n].astype(np.float64)
    c = (g - 4.5) * 8.0 + rng.uniform(-1.0, 1.0, (n, 3))
    r = rng.uniform(0.5, 1.5, n)
    rays = np.where((np.arange(n) % 2 == 0)[:, None], _through(rng, c, r, n, spread=0.7, far=(1.5, 3.0)), _inside(rng, c, r, n))
    j = rng.integers(-2, 3, n)
    addr = np.stack([np.arange(n), nodes, np.arange(n)], axis=1).astype(np.uint32)
    terms = L.medium_terms_v(rays, np.concatenate([c, r[:, None]], axis=1), np.ones(n), addr, seed)
    ok = (terms[:, 7] >= 2.0) & (terms[:, 4] > 0.0)          # the ray has a chord and a draw other than 0
    with np.errstate(all="ignore"):
        dens = np.where(ok, L.medium_neg_log_v(1.0 - terms[:, 4]) / (terms[:, 3] * (1.0 + j * EPS)), 1.0)
    dens = np.where(np.isfinite(dens) & (dens > 0.0), dens, 1.0)
    objs = [(c[i], r[i], "medium", dens[i]) for i in range(n)]
    return objs, rays, np.arange(n), {"j": j, "aimed": ok}


def _magnitudes(rng, w, L):
    n = N_R
    objs = []
    for _ in range(1 + int(rng.random() < 0.5)):
        objs.append((rng.standard_normal(3) * 10.0 ** rng.uniform(0.0, 6.0), 10.0 ** rng.uniform(-3.0, 4.0), "medium", 10.0 ** rng.uniform(-12.0, 12.0)))
    rays, target = _mixed_rays(rng, objs, list(range(len(objs))), n)
    d = rays[:, 3:]
    wild = rng.random(n) < 0.45
    scale = 10.0 ** rng.uniform(-150.0, 150.0, n)
    with np.errstate(all="ignore"):
        rays[:, 3:] = np.where(wild[:, None], d / np.linalg.norm(d, axis=1)[:, None] * scale[:, None], d)
    return objs, rays, target, {}


def _occluder_inside(rng, w, L):
    n = N_R
    c, R = rng.uniform(-5.0, 5.0, 3), rng.uniform(2.0, 4.0)
    co = c + _unit(rng, 1)[0] * R * rng.uniform(0.0, 0.5)
    ro = R * rng.uniform(0.1, 0.3)
    dens = np.log(2.0) / (0.7 * R) * rng.uniform(0.7, 1.4)
    medium, opaque = (c, R, "medium", dens), (co, ro, "opaque", 0.0)
    objs = [medium, opaque] if w % 2 == 0 else [opaque, medium]
    o = c + _unit(rng, n) * (R * rng.uniform(1.5, 4.0, n))[:, None]
    aim = co + rng.uniform(-1.0, 1.0, (n, 3)) * ro * 0.55
    rays = np.concatenate([o, (aim - o) * rng.uniform(0.3, 2.0, (n, 1))], axis=1)
    return objs, rays, np.full(n, w % 2, np.int64), {}


def _nested(rng, w, L):
    n = N_R
    c, r1 = rng.uniform(-5.0, 5.0, 3), rng.uniform(0.5, 1.5)
    r2 = r1 * rng.uniform(1.8, 3.0)
    inner, outer = (c, r1, "medium", 1.2 / r1 * rng.uniform(0.7, 1.4)), (c, r2, "medium", 0.35 / r2 * rng.uniform(0.7, 1.4))
    objs = [inner, outer] if w % 2 == 0 else [outer, inner]
    rays = _through(rng, c, r1, n, spread=0.8, far=(r2 / r1 * 1.2, r2 / r1 * 4.0))
    wide = _through(rng, c, r2, n, spread=1.6, far=(1.2, 4.0))
    ins = _inside(rng, c, r1, n)
    fam = rng.choice(3, n, p=[0.5, 0.25, 0.25])
    rays = np.where((fam == 1)[:, None], wide, np.where((fam == 2)[:, None], ins, rays))
    return objs, rays, np.full(n, w % 2, np.int64), {"inner": w % 2}


def _non_finite(rng, w, L):
    objs = _generic_objs(rng)
    rays, target = _mixed_rays(rng, objs, list(range(len(objs))), N_R)
    bad = np.array([np.nan, np.inf, -np.inf, 1e308, -1e308])
    hit = rng.random((N_R, 6)) < 0.15
    hit[np.arange(N_R), rng.integers(0, 6, N_R)] = True
    rays = np.where(hit, bad[rng.integers(0, len(bad), (N_R, 6))], rays)
    return objs, rays, target, {}


_DRAW = {"generic": _generic, "tangent": _tangent, "surface_origin": _surface_origin, "magnitudes": _magnitudes, "occluder_inside": _occluder_inside,
         "nested": _nested, "non_finite": _non_finite}
_worlds, _refs = {}, {}


def world_seed(cls, w):
    """the scene seed of world w: both key words in use from world 50 on"""
    return (0x5EED0000 + 977 * CLASSES.index(cls) + w) | ((w << 33) if w >= 50 else 0)


def class_worlds(cls, L):
    """the N_W worlds of a class, drawn once per session"""
    if cls not in _worlds:
        rng = np.random.default_rng(3000 + CLASSES.index(cls))
        out = []
        for w in range(N_W):
            seed = world_seed(cls, w)
            nodes = rng.choice(NODES, N_R)
            if cls == "boundary_density":
                objs, rays, target, notes = _boundary_density(rng, w, L, seed, nodes)
            else:
                objs, rays, target, notes = _DRAW[cls](rng, w, L)
            out.append(World(objs, rays, nodes, target, seed, **notes))
        _worlds[cls] = out
    return _worlds[cls]


class Reference:
    """the host build on a class: best, t (bits as f64), work over all N_W x N_R rays; took = the ray ends in a medium; terms = medium_terms_v
    of each ray against its target"""


def class_reference(cls, abi, L):
    if cls not in _refs:
        ref = Reference()
        best, t, work, took, terms = [], [], [], [], []
        with np.errstate(all="ignore"):
            for wd in class_worlds(cls, L):
                sc, keep = scene(abi, wd.objs, wd.seed)
                rc, b, tt, wk = L.hit_world_v(sc, wd.rays, node=wd.nodes)
                assert rc == 0, cls
                best.append(b); t.append(tt); work.append(wk)
                took.append((b >= 0) & wd.is_medium()[np.maximum(b, 0)])
                addr = np.stack([np.arange(len(wd.rays)), wd.nodes, wd.target], axis=1).astype(np.uint32)
                terms.append(L.medium_terms_v(wd.rays, wd.spheres4(), wd.densities(), addr, wd.seed))
        ref.best, ref.t, ref.work, ref.took, ref.terms = (np.concatenate(x) for x in (best, t, work, took, terms))
        for a in (ref.best, ref.t, ref.work, ref.took, ref.terms):
            a.setflags(write=False)
        _refs[cls] = ref
    return _refs[cls]


# ------------------------------------------------------------------ the adversarial walk worlds (tests/test_medium_cpu.py)
def _inside_rays(rng, centres, radii, media, count):
    """rays whose origin lies deep inside a medium (within 0.4 r of its centre: cells fully inside the ball for the big ones), short
    and long directions"""
    rays = np.zeros((count, 6))
    for k in range(count):
        j = int(media[k % len(media)])
        n = rng.standard_normal(3); n /= np.linalg.norm(n)
        rays[k, :3] = centres[j] + n * radii[j] * rng.uniform(0.0, 0.4)
        rays[k, 3:] = rng.standard_normal(3) * 10.0 ** rng.uniform(-2, 2)
    return rays


def _through_rays(rng, centres, radii, media, count):
    """rays from outside aimed through the heart of a medium: with a small density the candidate lies several cells past the first
    cell that lists the sphere"""
    rays = np.zeros((count, 6))
    for k in range(count):
        j = int(media[k % len(media)])
        n = rng.standard_normal(3); n /= np.linalg.norm(n)
        o = centres[j] + n * radii[j] * rng.uniform(1.5, 6.0)
        rays[k, :3] = o
        rays[k, 3:] = (centres[j] + rng.uniform(-0.3, 0.3, 3) * radii[j] - o) * rng.uniform(0.2, 2.0)
    return rays


WALK_WORLDS = {
    # (adversarial world, moving, environment): static / moving media, the packed tables and the wide ones
    "static": (0, False, {}),
    "static_ground": (1, False, {}),
    "big_radii": (3, False, {}),
    "moving": (0, True, {}),
    "moving_layer": (4, True, {}),
    "wide_tables": (0, False, {"RT_GRID_WIDE": "1"}),
    "thin_cells": (3, False, {"RT_GRID_N": "48,48,48"}),
}


class WalkWorld:
    """one of WALK_WORLDS as tests/test_medium_cpu.py draws it: the adversarial world with a quarter of its ordinary spheres made media
    (positive radius), some thin and some dense, three of them BIG so that they cover many cells, interior ones included; moving worlds at
    three shutter times; the ray families of tests/adversarial_rays.py, rays that start deep inside a medium, and rays whose candidate lies
    cells past the first listing.  `env` must be in the environment while tables are built from it."""

    def __init__(self, abi, name):
        wi, moving, env = WALK_WORLDS[name]
        rng = np.random.default_rng(9100 + sorted(WALK_WORLDS).index(name))
        sc, spheres, n = AR.adversarial_world(abi, rng, wi)
        sc.seed = 0x1234567 + wi
        tot = len(spheres)
        media = [i for i in range(n) if i % 4 == 1]
        for i in media:
            spheres[i].radius = abs(spheres[i].radius)
            spheres[i].kind = abi.RT_MAT_MEDIUM
            spheres[i].fuzz_or_ior = float(10.0 ** rng.uniform(-1.5, 1.5))
            spheres[i].albedo[:] = [0.5, 0.5, 0.5]
        for i in media[:3]:
            spheres[i].radius = spheres[i].radius * 4.0 + 1.0
            spheres[i].fuzz_or_ior = float(rng.uniform(0.05, 0.3))
        c0, radii = AR.sphere_arrays(spheres, tot)
        dens = np.array([spheres[i].fuzz_or_ior if spheres[i].kind == abi.RT_MAT_MEDIUM else 0.0 for i in range(tot)])
        c1 = c0.copy()
        if moving:
            for i in range(n):
                if i % 3 != 2:
                    c1[i] = c0[i] + rng.uniform(-0.7, 0.7, 3)
        dv = np.where(c1 == c0, -0.0, c1 - c0)
        blocks = []
        for tau in ([0.0] if not moving else [0.0, 1.0 - 2.0 ** -24, float(np.float32(rng.integers(0, 1 << 24) * 2.0 ** -24))]):
            ct = c0 + dv * np.float64(tau)
            moved = (abi.RtSphere * tot)()
            C.memmove(moved, spheres, C.sizeof(moved))
            for i in range(tot):
                moved[i].center[:] = list(ct[i])
            per = 84 if moving else 210
            rays = np.concatenate([AR.ray_table(rng, moved, n, per, list(range(AR.FAMILIES)))[0],
                                   _inside_rays(rng, ct, radii, media, per // 3), _through_rays(rng, ct, radii, media, per // 3)])
            blocks.append((tau, ct, rays))
        self.name, self.wi, self.moving, self.env = name, wi, moving, env
        self.sc, self.spheres, self.n, self.tot, self.media = sc, spheres, n, tot, media
        self.c0, self.c1, self.radii, self.dens, self.blocks = c0, c1, radii, dens, blocks
        self.c1c = np.ascontiguousarray(c1) if moving else None
        self.rays = np.ascontiguousarray(np.concatenate([b[2] for b in blocks]))
        self.tau = np.concatenate([np.full(len(b[2]), b[0], np.float32) for b in blocks])
        self.nodes = np.ascontiguousarray(rng.choice(NODES, len(self.rays)))
