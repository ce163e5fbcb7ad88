"""Random worlds and adversarial rays for the grid walk, shared by the CPU checks of its host build (test_core_cpu.py, through
tests/hostsim) and the GPU checks of the megakernel's walk (test_walk_rays_gpu.py).

The seven families of test_core_cpu.py's test_grid_walk_adversarial_rays (FAMILIES, drawn from the same generator in the same
order: a seed gives the same rays it always gave) plus two that need the grid's geometry (hostsim_grid_geom):
  CELL_PLANE  the origin lies on a plane between cells and the direction's component along that axis is exactly +-0: the
              ray runs inside the plane, its slab parameters along that axis are +-inf;
  CELL_EDGE   the origin lies on a cell edge or corner: rays along the edge (two zero components), and rays whose direction is
              one cell along every axis, which cross every later plane exactly at a corner (three-way ties of the DDA)."""
import ctypes as C

import numpy as np

# the worlds of test_grid_walk_adversarial_rays, in its order (adversarial_world shapes 1, 3 and 4 further)
WORLDS = [dict(n=200, spread=5.0, r_lo=0.05, r_hi=0.6, big=None), dict(n=600, spread=20.0, r_lo=0.1, r_hi=0.3, big=1000.0),
          dict(n=80, spread=1.0, r_lo=0.2, r_hi=0.5, big=None), dict(n=300, spread=8.0, r_lo=0.01, r_hi=2.5, big=None),
          dict(n=900, spread=25.0, r_lo=0.2, r_hi=0.2, big=1000.0)]
FAMILIES = 7                 # kinds 0 .. 6 of adversarial_ray
CELL_PLANE, CELL_EDGE = 7, 8
ALL_KINDS = FAMILIES + 2


def random_scene(abi, rng, n, spread, r_lo, r_hi, big=None):
    """n Lambertian spheres (every 11th with a negative radius) in a cube of side 2 * spread, plus a ground sphere of radius big"""
    spheres = (abi.RtSphere * (n + (1 if big else 0)))()
    for i in range(n):
        c = rng.uniform(-spread, spread, 3)
        spheres[i].center[:] = list(c)
        spheres[i].radius = float(rng.uniform(r_lo, r_hi)) * (-1.0 if i % 11 == 0 else 1.0)
        spheres[i].kind = abi.RT_MAT_LAMBERTIAN
    if big:
        spheres[n].center[:] = [0.0, -big - spread, 0.0]
        spheres[n].radius = big
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=4, height=4, samples_per_pixel=1, max_depth=2,
                     spheres=spheres, n_spheres=len(spheres))
    return sc, spheres


def adversarial_world(abi, rng, wi):
    """world wi of WORLDS -> (RtScene, spheres array, number of ordinary spheres)"""
    wd = WORLDS[wi]
    sc, spheres = random_scene(abi, rng, **wd)
    if wi == 1:  # flat world: every centre near y = 0
        for i in range(wd["n"]):
            spheres[i].center[1] = float(rng.uniform(0.0, 0.3))
    if wi == 4:  # exactly one layer of equal spheres on the ground: the grid is a single cell high
        for i in range(wd["n"]):
            spheres[i].center[1] = 0.2
            spheres[i].radius = 0.2
    if wi == 3:  # far from the origin: large coordinates, small spheres
        for i in range(wd["n"]):
            for k in range(3):
                spheres[i].center[k] += 5000.0
    return sc, spheres, wd["n"]


def grid_geometry(hostsim, scene_ptr):
    """(gmin[3], cell size[3], cells per axis[3]) of the grid the table builder makes for a scene (C.byref(RtScene) or a
    POINTER(RtScene)); honours RT_GRID_N / RT_GRID_WIDE like the libraries built with the test probes"""
    info = (C.c_uint32 * 6)()
    geom = (C.c_double * 6)()
    assert hostsim.hostsim_grid_info(scene_ptr, info) == 0 and info[0] > 0, "world must be gridded"
    assert hostsim.hostsim_grid_geom(scene_ptr, geom) == 0
    return np.array(geom[0:3]), np.array(geom[3:6]), np.array(info[0:3], np.int64)


def adversarial_ray(rng, spheres, n, kind, grid=None):
    """one ray (origin, direction) of family `kind` aimed at one of the first n spheres; CELL_PLANE and CELL_EDGE need
    grid = grid_geometry(...)"""
    i = int(rng.integers(n))
    c = np.array(spheres[i].center[:]); r = abs(spheres[i].radius)
    nrm = rng.standard_normal(3); nrm /= np.linalg.norm(nrm)
    if kind == 0:    # leaves a sphere surface in a random direction (a bounced ray)
        o = c + nrm * r; d = rng.standard_normal(3)
    elif kind == 1:  # grazes sphere i: offset from the centre ~ r (1 +- tiny)
        tdir = np.cross(nrm, rng.standard_normal(3)); tdir /= np.linalg.norm(tdir)
        p = c + nrm * r * (1.0 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-15, -2))
        o = p - tdir * rng.uniform(0.5, 30.0); d = tdir * rng.uniform(0.1, 3.0)
    elif kind == 2:  # axis-parallel through the sphere's bounding box
        ax = int(rng.integers(3)); d = np.zeros(3); d[ax] = rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 2.0)
        o = c + rng.uniform(-1.2, 1.2, 3) * r; o[ax] -= np.sign(d[ax]) * rng.uniform(1.0, 40.0)
    elif kind == 3:  # from far outside the grid towards a sphere
        o = c + nrm * 10.0 ** rng.uniform(1, 4.5); d = (c + rng.uniform(-1, 1, 3) * r * 1.5) - o
    elif kind == 4:  # one direction component denormal / zero, the others diagonal
        d = rng.choice([-1.0, 1.0], 3); d[int(rng.integers(3))] = rng.choice([0.0, -0.0, 1e-310, -1e-300, 1e-40])
        o = c - d * rng.uniform(0.5, 10.0) + rng.uniform(-1, 1, 3) * r
    elif kind == 5:  # starts inside a sphere
        o = c + nrm * r * rng.uniform(0.0, 0.999); d = rng.standard_normal(3) * 10.0 ** rng.uniform(-3, 3)
    elif kind == 6:  # hits sphere i at (almost) its extreme point along an axis — for the outermost
                     # spheres that is on the grid's outer face — coming in nearly parallel to that face
        ax = int(rng.integers(3)); sgn = rng.choice([-1.0, 1.0])
        e = np.zeros(3); e[ax] = sgn
        p = c + e * r * (1.0 - 10.0 ** rng.uniform(-12, -2))
        tdir = rng.standard_normal(3); tdir[ax] = 0.0; tdir /= np.linalg.norm(tdir)
        d = tdir + e * 10.0 ** rng.uniform(-4, -1.5)
        o = p - d * rng.uniform(0.5, 12.0)
    else:
        gmin, size, ncell = grid

        def plane(ax, x):  # the face plane of the grid along axis ax nearest to coordinate x, moved by -1, 0 or +1 cells
            j = int(np.clip(np.rint((x - gmin[ax]) / size[ax]) + rng.integers(-1, 2), 0, ncell[ax]))
            return gmin[ax] + j * size[ax]
        if kind == CELL_PLANE:   # inside the plane: d[ax] = +-0 exactly; the other components aimed near sphere i
            ax = int(rng.integers(3))
            tdir = rng.standard_normal(3); tdir[ax] = 0.0; tdir /= np.linalg.norm(tdir)
            p = c + rng.uniform(-1.5, 1.5, 3) * r
            o = p - tdir * 10.0 ** rng.uniform(-0.5, 3.0)
            o[ax] = plane(ax, c[ax])
            d = tdir * 10.0 ** rng.uniform(-2, 2)
            d[ax] = rng.choice([0.0, -0.0])
        else:                    # CELL_EDGE: from a cell edge / corner near sphere i
            o = np.array([plane(k, c[k] + rng.uniform(-1.5, 1.5) * r) for k in range(3)])
            if rng.random() < 0.5:   # along the edge: two components exactly +-0, the ray lies in two planes
                ax = int(rng.integers(3))
                d = np.array([rng.choice([0.0, -0.0]) for _ in range(3)])
                d[ax] = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-2, 2)
                o[ax] = c[ax] - np.sign(d[ax]) * rng.uniform(0.0, 20.0) * max(r, size[ax])
            else:                    # one cell along every axis: the ray crosses the later planes at corners
                d = rng.choice([-1.0, 1.0], 3) * size * float(rng.integers(1, 4))
    return o, d


def ray_table(rng, spheres, n, count, kinds, grid=None):
    """count rays of the given families, round robin -> (count x 6 f64 {origin, direction}, family of each)"""
    rays = np.zeros((count, 6))
    fam = np.zeros(count, np.int32)
    for k in range(count):
        kind = kinds[k % len(kinds)]
        o, d = adversarial_ray(rng, spheres, n, kind, grid)
        rays[k, :3], rays[k, 3:] = o, d
        fam[k] = kind
    return rays, fam


def hit_world_v(hostsim, scene_ptr, rays, work=None):
    """tests/hostsim's hit_world_grid and its brute force over n rays (n x 6) -> (best grid, t grid, best brute, t brute);
    work: an n x 2 uint32 array that receives each walk's {exact tests, grid steps}"""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    best = np.zeros((n, 2), np.int32)
    t = np.zeros((n, 2), np.float64)
    if work is not None:
        assert work.dtype == np.uint32 and work.shape == (n, 2) and work.flags.c_contiguous
    assert hostsim.hostsim_hit_world_v(scene_ptr, C.c_void_p(rays.ctypes.data), C.c_uint64(n), C.c_void_p(best.ctypes.data),
                                       C.c_void_p(t.ctypes.data), C.c_void_p(work.ctypes.data if work is not None else None)) == 0
    return best[:, 0], t[:, 0], best[:, 1], t[:, 1]


F64_MAX = np.finfo(np.float64).max
T_MIN = 0.001   # raytracer.rs:84


def sphere_hit_t(o, d, centres, radii, t_min=T_MIN):
    """Sphere::hit (sphere.rs:46-58) with t_max = f64::MAX, in numpy f64 with the operation order of the oracle's sphere_hit:
    o, d (n x 3) against centres (m x 3), radii (m) -> n x m accepted roots, +inf where the sphere is missed (the near root,
    else the far one, each only above t_min)"""
    dx, dy, dz = (d[:, k:k + 1] for k in range(3))
    a = (dx * dx + dy * dy) + dz * dz
    ocx, ocy, ocz = (o[:, k:k + 1] - centres[None, :, k] for k in range(3))
    half_b = (ocx * dx + ocy * dy) + ocz * dz
    c = ((ocx * ocx + ocy * ocy) + ocz * ocz) - radii[None, :] * radii[None, :]
    disc = (half_b * half_b) - (a * c)
    ok = disc >= 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sq = np.sqrt(np.where(ok, disc, 0.0))
        near = ((-half_b) - sq) / a
        far = ((-half_b) + sq) / a
    t = np.where(ok & (near < F64_MAX) & (near > t_min), near, np.where(ok & (far < F64_MAX) & (far > t_min), far, np.inf))
    return t


def brute_force_hit_world(rays, centres, radii, chunk=256):
    """hit_world (raytracer.rs:44-59) by brute force: the object-order scan keeps a root only when it is below the closest so
    far, so the result is the smallest accepted root and, among equal roots, the lowest index -> (best (-1: none), t
    (f64::MAX: none)) per ray"""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    o, d = rays[:, :3], rays[:, 3:]
    best = np.full(len(rays), -1, np.int32)
    t = np.full(len(rays), F64_MAX)
    for s0 in range(0, len(radii), chunk):
        tc = sphere_hit_t(o, d, centres[s0:s0 + chunk], radii[s0:s0 + chunk])
        i = np.argmin(tc, axis=1)
        tm = tc[np.arange(len(rays)), i]
        take = tm < t   # (strict: an earlier chunk keeps a tie)
        best[take] = (s0 + i[take]).astype(np.int32)
        t[take] = tm[take]
    return best, t


def sphere_arrays(spheres, n):
    """(centres n x 3, radii n) of the first n records of an RtSphere array"""
    centres = np.array([spheres[i].center[:] for i in range(n)], np.float64).reshape(n, 3)
    radii = np.array([spheres[i].radius for i in range(n)], np.float64)
    return centres, radii
