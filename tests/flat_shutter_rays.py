"""The ray tables of the shutter probe's tests, shared by the host build's test (tests/test_flat_shutter_cpu.py) and the device's
(tests/test_flat_shutter_gpu.py): worlds of flat primitives that move within the frame, every ray with its own shutter time, closest-so-far
and — in the `held` worlds — the hit it already holds.  TEST INFRASTRUCTURE: seeded, computed once per process, read-only.

A world is a dict: quvs (n x 9), shapes (n, u32: 0 parallelogram, 1 triangle), move (n x 3, or None), normals (n x 9, or None), rays (m x 6),
tau (m, f32), closest (m), best_in (m, i32, or None) and aim (m: the entry a ray was made for).  Entry k is object ID_BASE + k: the device
scene holds one sphere, which no ray of the probe is ever tested against."""
import functools

import numpy as np

import quad_rays as QR
import smooth_points as SP

ID_BASE = 1
T_MAX = QR.T_MAX
PER_ENTRY = 100                       # the first 100 rays of each entry's batch (an axis class: the first 10 000 of its one batch)
HELD_CLASSES = ("generic", "edges", "t_range")
TIE_KINDS = ("larger", "smaller", "sphere")


def _freeze(w):
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def full_class_world(abi, cls):
    """one list per class of tests/quad_rays.py: the class's entries a device scene can hold (filled up to 100 with generic ones; triangles
    and parallelograms in turn, every other entry moving by about its own size) and all its rays, each with its own tau and moved along
    with the entry it is aimed at -> quvs, shapes, move, rays, tau, closest (the tables' own), aim"""
    import lane_sim
    rng = np.random.default_rng(5100 + QR.CLASSES.index(cls))
    quvs, rays, closest, aim = [], [], [], []
    for quv, r, c in QR.device_class_tables(cls, lane_sim.load(abi)):
        quvs.append(quv); rays.append(r); closest.append(c); aim += [len(quvs) - 1] * len(r)
    if len(quvs) < 100:
        quvs += list(QR._quads(rng, 100 - len(quvs)))
    quvs, rays, closest, aim = np.array(quvs), np.concatenate(rays), np.concatenate(closest), np.array(aim)
    n = len(quvs)
    shapes = (np.arange(n) % 2).astype(np.uint32)
    move = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        move[::2] = (rng.uniform(-1.0, 1.0, (n, 3)) * np.linalg.norm(quvs[:, 3:6], axis=1)[:, None])[::2]
        tau = (rng.integers(0, 1 << 24, len(rays)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
        tau[::3], tau[1::3] = 0.0, np.float32(1.0 - 2.0 ** -24)
        rays[:, :3] = rays[:, :3] + move[aim] * tau[:, None].astype(np.float64)
    return quvs, shapes, move, rays, tau, closest, aim


@functools.lru_cache(maxsize=None)
def class_world(abi, cls):
    """full_class_world(cls) reduced to 10^4 rays, each with the table's own closest-so-far: taus of 0, 1 - 2^-24 and random multiples
    of 2^-24"""
    quvs, shapes, move, rays, tau, closest, aim = full_class_world(abi, cls)
    if cls in QR.AXIS_CLASSES:
        keep = np.arange(100 * PER_ENTRY)
    else:
        keep = (np.arange(100)[:, None] * QR.N_R + np.arange(PER_ENTRY)[None, :]).reshape(-1)
    assert len(rays) >= 100 * QR.N_R and len(keep) == 10_000
    pick = lambda a: np.ascontiguousarray(a[keep])
    return _freeze(dict(quvs=quvs, shapes=shapes, move=move, normals=None, rays=pick(rays), tau=pick(tau), closest=pick(closest), best_in=None,
                        aim=pick(aim)))


@functools.lru_cache(maxsize=None)
def held_world(abi, cls):
    """class_world(cls) whose rays come with a hit already held: best_in drawn per ray from {-1, 0 (the sphere), a flat id below the true
    hit, a flat id above it}, closest set to the ray's true t in half of the rays — `true` from a first pass of the host build with nothing
    held and no bound — so exact ties against a larger index, a smaller index and a sphere all occur.  Adds tie (m: -1, or the index into
    TIE_KINDS of the tie the ray makes), true_best and true_t."""
    import flat_motion_sim
    w = dict(class_world(abi, cls))
    import flat_bvh_sim as F
    flats = F.flats_array(abi, w["quvs"], w["shapes"])
    m, n = len(w["rays"]), len(w["quvs"])
    first, _ = flat_motion_sim.load(abi).list_surface(flats, w["move"], w["rays"], w["tau"], np.full(m, T_MAX), False, id_base=ID_BASE)
    rng = np.random.default_rng(5300 + QR.CLASSES.index(cls))
    hit = first["best"] >= ID_BASE
    k = np.where(hit, first["best"] - ID_BASE, rng.integers(0, n, m))          # (a ray that hits nothing: about a random entry)
    kind = rng.integers(0, 4, m)
    below = ID_BASE + (rng.random(m) * k).astype(np.int64)                     # a flat id in [ID_BASE, ID_BASE + k)
    above = ID_BASE + k + 1 + (rng.random(m) * (n - 1 - k)).astype(np.int64)   # ... in (ID_BASE + k, ID_BASE + n)
    kind = np.where((kind == 2) & (k == 0), 0, np.where((kind == 3) & (k == n - 1), 0, kind))
    best_in = np.select([kind == 0, kind == 1, kind == 2], [-1, 0, below], above).astype(np.int32)
    tied = hit & (rng.random(m) < 0.5)
    closest = np.where(tied, first["t"], w["closest"])
    tie = np.where(tied & (kind == 3), 0, np.where(tied & (kind == 2), 1, np.where(tied & (kind == 1), 2, -1)))
    w.update(closest=closest, best_in=best_in, tie=tie, true_best=first["best"].copy(), true_t=np.where(hit, first["t"], np.nan))
    return _freeze(w)


SMOOTH_CLASSES = (("generic", 50), ("edges", 30), ("opposite", 30), ("side", 30), ("grazing", 30), ("needle", 30))
SMOOTH_REP = 50


@functools.lru_cache(maxsize=None)
def smooth_world(abi=None):
    """200 triangles of tests/smooth_points.py's classes — the degenerate-normal ones included — with their vertex normals and 50 rays on
    each, o = P - d as its device tables make them; every other entry moves by about its own size and its rays move along.  Adds cls (m:
    the index into SMOOTH_CLASSES of the ray's class).  A caller leaves out `move` or `normals` to get the other two scenes of the three."""
    rng = np.random.default_rng(5400)
    quvs, normals, rays, aim, cls_of = [], [], [], [], []
    for ci, (cls, ne) in enumerate(SMOOTH_CLASSES):
        quv, nr, d, P = SP._gen(cls, rng, ne, SMOOTH_REP)
        aim.append(sum(len(q) for q in quvs) + np.repeat(np.arange(ne), SMOOTH_REP))
        quvs.append(quv[::SMOOTH_REP]); normals.append(nr[::SMOOTH_REP]); rays.append(np.concatenate([P - d, d], axis=1))
        cls_of.append(np.full(ne * SMOOTH_REP, ci))
    quvs, normals, rays, aim, cls_of = (np.concatenate(x) for x in (quvs, normals, rays, aim, cls_of))
    n, m = len(quvs), len(rays)
    assert n == 200 and m == 200 * SMOOTH_REP
    move = np.zeros((n, 3))
    move[::2] = (rng.uniform(-1.0, 1.0, (n, 3)) * np.linalg.norm(quvs[:, 3:6], axis=1)[:, None])[::2]
    tau = (rng.integers(0, 1 << 24, m).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    tau[::5], tau[1::5] = 0.0, np.float32(1.0 - 2.0 ** -24)
    rays[:, :3] = rays[:, :3] + move[aim] * tau[:, None].astype(np.float64)
    closest = np.where(rng.random(m) < 0.5, T_MAX, rng.uniform(0.5, 4.0, m))
    return _freeze(dict(quvs=np.ascontiguousarray(quvs), shapes=np.ones(n, np.uint32), move=move, normals=np.ascontiguousarray(normals),
                        rays=np.ascontiguousarray(rays), tau=tau, closest=closest, best_in=None, aim=aim, cls=cls_of))


@functools.lru_cache(maxsize=None)
def still_world(abi):
    """class_world("generic") with every displacement zero, plus entry 100: a speck of 1 mm a million units away that moves by 2 mm and that
    no ray reaches, so the scene keeps its motion table and every still entry goes through the moving code; and entries 101 and 102, whose
    origins are zeros of either sign, with 100 rays each: q + (-0.0) tau must give q's own bits back"""
    w = class_world(abi, "generic")
    rng = np.random.default_rng(5500)
    speck = np.array([1e6, 1e6, 1e6, 0.001, 0.0, 0.0, 0.0, 0.001, 0.0])
    zeros = np.array([[-0.0, 0.0, -0.0, 3.0, 0.0, 0.0, 0.0, 3.0, 0.0], [0.0, -0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.5, 2.0]])
    extra = np.concatenate([QR._aimed(rng, q, 100, dist=(0.05, 0.5)) for q in zeros])
    m = len(extra)
    tau = (rng.integers(0, 1 << 24, m).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    move = np.zeros((103, 3)); move[100] = [0.0, 0.002, 0.0]
    return _freeze(dict(quvs=np.concatenate([w["quvs"], speck[None, :], zeros]), shapes=np.concatenate([w["shapes"], [0, 0, 1]]).astype(np.uint32),
                        move=move, normals=None, rays=np.concatenate([w["rays"], extra]), tau=np.concatenate([w["tau"], tau]),
                        closest=np.concatenate([w["closest"], np.full(m, T_MAX)]), best_in=None, aim=np.concatenate([w["aim"], np.repeat([101, 102], 100)])))


@functools.lru_cache(maxsize=None)
def image_world():
    """16 parallelograms with 8 x 8 images — two textures whose red tells the texel, the four combinations of wrap modes, (s, t) corners
    drawn from [-1.5, 2.5] — every other one moving, 64 rays aimed inside each and moved along with it.  Adds textures (two [8, 8, 3] u8),
    uvs (per entry, six floats) and modes (per entry: wrap_s, wrap_t); entry k shows texture k % 2."""
    rng = np.random.default_rng(5600)
    n, per = 16, 64
    quvs = QR._quads(rng, n)
    textures = []
    for _ in range(2):
        a = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
        a[..., 0] = np.arange(64).reshape(8, 8) * 4 + 1                     # (red tells the texel)
        textures.append(np.ascontiguousarray(a))
    move = np.zeros((n, 3))
    move[::2] = (rng.uniform(-1.0, 1.0, (n, 3)) * np.linalg.norm(quvs[:, 3:6], axis=1)[:, None])[::2]
    aim = np.repeat(np.arange(n), per)
    rays = np.concatenate([QR._aimed(rng, q, per, ab=rng.uniform(0.02, 0.98, (per, 2))) for q in quvs])
    tau = (rng.integers(0, 1 << 24, len(rays)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    rays[:, :3] += move[aim] * tau[:, None].astype(np.float64)
    modes = [(k % 2, (k // 2) % 2) for k in range(n)]
    uvs = [tuple(rng.uniform(-1.5, 2.5, 6).tolist()) for _ in range(n)]
    for a in textures:
        a.setflags(write=False)
    return _freeze(dict(quvs=quvs, shapes=np.zeros(n, np.uint32), move=move, normals=None, rays=rays, tau=tau, closest=np.full(len(rays), T_MAX),
                        best_in=None, aim=aim, textures=textures, uvs=uvs, modes=modes))


def flats(abi, w):
    """the world's entries as a ctypes array of abi.RtQuad"""
    import flat_bvh_sim as F
    return F.flats_array(abi, w["quvs"], w["shapes"])


def host_pass(abi, w, bvh, move="world", normals="world", out=None):
    """the host build's answer for a world (tests/flat_motion_sim.py list_surface) -> outputs, counts"""
    import flat_motion_sim
    return flat_motion_sim.load(abi).list_surface(flats(abi, w), w["move"] if isinstance(move, str) else move, w["rays"], w["tau"], w["closest"], bvh,
                                                  id_base=ID_BASE, best_in=w["best_in"], normals=w["normals"] if isinstance(normals, str) else normals,
                                                  out=out)


SENTINEL = dict(best=-7, t=-1.25, P=-2.5, normal=-3.75, front=-9, origin=-5.5)


def sentinels(m):
    """the outputs pre-filled: what a ray that accepts no new flat entry must leave as it was (best is always written)"""
    return dict(best=np.full(m, SENTINEL["best"], np.int32), t=np.full(m, SENTINEL["t"]), P=np.full((m, 3), SENTINEL["P"]),
                normal=np.full((m, 3), SENTINEL["normal"]), front=np.full(m, SENTINEL["front"], np.int32), origin=np.full((m, 3), SENTINEL["origin"]))


def accepted(w, best):
    """the rays whose outputs are written: the id returned is a flat entry and not the hit the ray came with"""
    held = w["best_in"] if w["best_in"] is not None else np.full(len(best), -1, np.int32)
    return (best >= ID_BASE) & (best != held)
