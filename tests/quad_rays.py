"""The ray tables of the quad code's bit tests, shared by the host build's test (tests/test_quad_cpu.py) and the device's
(tests/test_quad_rays_gpu.py): nine classes of (quad, rays, closest-so-far), >= 10^5 rays each, each aimed at one decision of
csrc/common/rt_quad.h.  class_tables(cls) yields the batches (quv = q, u, v as 9 doubles; rays n x 6; closest n) with fixed seeds;
device_class_tables(cls) the same batches restricted to quads a scene can hold."""
import numpy as np

T_MAX = 1.7976931348623157e308
AXIS_QUV = np.array([-1.0, -2.0, 0.5, 4.0, 0.0, 0.0, 0.0, 2.0, 0.0])     # N = (0, 0, 1), D = 0.5 exactly: den = d_z, t = (0.5 - o_z) / d_z
CLASSES = ["generic", "den", "edges", "on_plane", "t_range", "magnitudes", "non_finite", "skewed", "needle"]
AXIS_CLASSES = ("den", "t_range")             # one batch of N_Q x N_R rays against AXIS_QUV; every other class: N_Q quads x N_R rays
STRADDLING = tuple(c for c in CLASSES if c not in ("magnitudes", "non_finite", "on_plane"))   # 5 % .. 95 % of these classes' rays hit
N_Q, N_R = 100, 1000


def _quads(rng, n, kind="generic"):
    q = rng.uniform(-8.0, 8.0, (n, 3))
    u = rng.standard_normal((n, 3)) * rng.uniform(0.5, 4.0, (n, 1))
    v = rng.standard_normal((n, 3)) * rng.uniform(0.5, 4.0, (n, 1))
    if kind == "skewed":      # nearly parallel edges: a sliver of a parallelogram
        v = u * rng.uniform(0.3, 2.0, (n, 1)) + rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-6, -1, (n, 1))
    if kind == "needle":      # one edge 10^3 .. 10^8 times the other
        v = v * 10.0 ** rng.uniform(-8, -3, (n, 1))
    return np.concatenate([q, u, v], axis=1)


def _aimed(rng, quv, n, ab=None, dist=(0.5, 16.0)):
    """n rays aimed at Q + a u + b v (a, b given or uniform in [-0.5, 1.5]) from random origins, d = (target - o) * a random scale"""
    if ab is None:
        ab = rng.uniform(-0.5, 1.5, (n, 2))
    target = quv[0:3] + ab[:, :1] * quv[3:6] + ab[:, 1:] * quv[6:9]
    dirs = rng.standard_normal((n, 3))
    o = target - dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(*dist, (n, 1))
    return np.concatenate([o, (target - o) * rng.uniform(0.25, 4.0, (n, 1))], axis=1)


def _ulps(x, k):
    """x moved by k units in the last place (k an integer array, either sign)"""
    b = np.ascontiguousarray(x, np.float64).view(np.int64)
    return (b + np.where(x >= 0, k, -k)).view(np.float64)


def _batches(cls, rng, n_q, n_r):
    """the batches of one round of a class from rng: n_q quads drawn first, then each quad's rays (or the single batch of an axis class)"""
    if cls not in AXIS_CLASSES:
        kind = cls if cls in ("skewed", "needle") else "generic"
        for quv in _quads(rng, n_q, kind):
            closest = np.where(rng.random(n_r) < 0.5, T_MAX, rng.uniform(0.0, 8.0, n_r))
            if cls == "edges":       # through the four edges and corners: a, b within a few ulps of 0 and 1 (and exactly there)
                ab = rng.uniform(-0.2, 1.2, (n_r, 2))
                k = rng.integers(-4, 5, (n_r, 2))
                edge = np.where(rng.random((n_r, 2)) < 0.5, _ulps(np.ones((n_r, 2)), k), k * 2.0 ** -54)
                ab = np.where(rng.integers(0, 3, (n_r, 2)) > 0, edge, ab)
                rays = _aimed(rng, quv, n_r, ab)
            elif cls == "on_plane":  # origins on the plane (t = 0 up to rounding), any direction; some an exact vertex
                ab = rng.uniform(-0.5, 1.5, (n_r, 2))
                o = quv[0:3] + ab[:, :1] * quv[3:6] + ab[:, 1:] * quv[6:9]
                o[:10] = quv[0:3]
                rays = np.concatenate([o, rng.standard_normal((n_r, 3))], axis=1)
            else:
                rays = _aimed(rng, quv, n_r)
            if cls == "magnitudes":  # huge and tiny |d| (t scales inversely), huge and tiny quads and distances
                rays[:, 3:] *= 10.0 ** rng.uniform(-300, 300, (n_r, 1))
                s = 10.0 ** rng.uniform(-100, 100)
                quv, rays[:, :3] = quv * s, rays[:, :3] * s
                rays[:, 3:] *= np.where(rng.random((n_r, 1)) < 0.5, s, 1.0)
            if cls == "non_finite":
                bad = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e308, -1e308, 5e-324])
                sel = rng.random((n_r, 6)) < 0.15
                rays = np.where(sel, bad[rng.integers(0, len(bad), (n_r, 6))], rays)
                closest = np.where(rng.random(n_r) < 0.2, bad[rng.integers(0, len(bad), n_r)], closest)
            yield quv, rays, closest
    else:
        n = n_q * n_r
        o = np.concatenate([rng.uniform(-3.0, 5.0, (n, 2)), rng.uniform(-4.0, 4.0, (n, 1))], axis=1)
        d = rng.standard_normal((n, 3))
        closest = np.full(n, T_MAX)
        if cls == "den":         # den = d_z within a few ulps of +-1e-8 on both sides (and exactly there), and of 0
            d[:, 2] = _ulps(np.where(rng.random(n) < 0.5, 1e-8, -1e-8), rng.integers(-6, 7, n))
            d[: n // 20, 2] = rng.integers(-3, 4, n // 20) * 5e-324
            o[:, 2] = 0.5 - d[:, 2] * rng.uniform(0.5, 2.0, n) * np.where(rng.random(n) < 0.9, 1.0, 1e8)   # t = 0.5 .. 2 (or 1e8: far off the quad)
            d[:, :2] = (rng.uniform(-1.0, 3.0, (n, 2)) * [1.0, 0.5] + [0.0, -1.5] - o[:, :2]) / ((0.5 - o[:, 2]) / d[:, 2])[:, None]
        else:                    # t within a few ulps of 0.001 and of closest, on both sides (and exactly there)
            d[:, 2] = np.where(rng.random(n) < 0.5, 1.0, -2.0)
            near_min = rng.random(n) < 0.5
            t = np.where(near_min, _ulps(np.full(n, 0.001), rng.integers(-6, 7, n)), rng.uniform(0.01, 4.0, n))
            o[:, 2] = 0.5 - t * d[:, 2]
            t_real = (0.5 - o[:, 2]) / d[:, 2]
            closest = np.where(near_min, closest, _ulps(t_real, rng.integers(-6, 7, n)))
            d[:, :2] = (rng.uniform(-1.0, 3.0, (n, 2)) * [1.0, 0.5] + [0.0, -1.5] - o[:, :2]) / t_real[:, None]
        yield AXIS_QUV, np.concatenate([o, d], axis=1), closest


def class_tables(cls):
    """(quv, rays, closest) batches of one class: 100 quads x 1 000 rays, or the axis-aligned quad whose den and t are exact functions of the
    ray with its 100 000 rays in one batch.  Some `magnitudes` quads are ones rt_quad_prepare refuses (nn overflows or underflows)."""
    yield from _batches(cls, np.random.default_rng(2000 + CLASSES.index(cls)), N_Q, N_R)


def device_class_tables(cls, sim=None):
    """class_tables(cls) for a device scene, which cannot hold a refused quad: for an axis class its batch; for every other class exactly
    100 batches whose quads the host build's rt_quad_prepare accepts (sim: the lane simulator, loaded here when not given).  Every class
    but `magnitudes` must have its first 100 accepted as drawn, so its table IS class_tables(cls); `magnitudes` (quads scaled by 10^+-100:
    about a quarter refused) goes on drawing rounds of 100 from the same generator, keeping the accepted ones in order."""
    if cls in AXIS_CLASSES:
        yield from class_tables(cls)
        return
    if sim is None:
        import lane_sim
        from conftest import graft
        sim = lane_sim.load(graft.load_package().abi)
    rng = np.random.default_rng(2000 + CLASSES.index(cls))
    kept = drawn = 0
    while kept < N_Q:
        for quv, rays, closest in _batches(cls, rng, N_Q, N_R):
            ok = int(sim.quad_prepare_v(quv[None, :])[1][0]) == 0
            drawn += 1
            assert ok or cls == "magnitudes", f"{cls}: quad {drawn - 1} is refused by rt_quad_prepare: {quv.tolist()}"
            if ok and kept < N_Q:
                kept += 1
                yield quv, rays, closest
                if kept == N_Q:
                    return
        assert drawn < 20 * N_Q, f"{cls}: {kept} of {drawn} quads accepted"
