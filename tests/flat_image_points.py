"""Tables of hits for the texel lookup of images on flat primitives: per class N hits, each with its own resident record,
frame (O, u, v, w) and point P.  Deterministic; the CPU test (host build against the restatement) and the GPU test (device build against
the host build) walk the same tables.  TEST INFRASTRUCTURE."""
import numpy as np

from flat_image_sim import REC, records

N = 100_000
CLASSES = ["triangle", "parallelogram", "integer_edges", "tiling", "clamp_far", "needles", "one_texel", "non_finite"]
SIZES = np.array([(8, 4), (5, 3), (1, 1), (640, 480), (3, 1000)], np.uint32)
_CACHE = {}


def _frame(rng, n, skew=None):
    """O, u, v and w = n / dot(n, n), n = cross(u, v), of n random entries"""
    O = rng.uniform(-5, 5, (n, 3))
    u = rng.uniform(-2, 2, (n, 3))
    v = rng.uniform(-2, 2, (n, 3))
    if skew is not None:                                   # needles: v nearly along u, and sides of very different length
        v = u * rng.uniform(0.5, 2.0, (n, 1)) + rng.uniform(-1, 1, (n, 3)) * skew
        u = u * 10.0 ** rng.uniform(-3, 3, (n, 1))
    nrm = np.cross(u, v)
    nn = (nrm * nrm).sum(axis=1, keepdims=True)
    keep = (nn[:, 0] > 1e-30)
    u[~keep], v[~keep] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    nrm = np.cross(u, v)
    nn = (nrm * nrm).sum(axis=1, keepdims=True)
    return O, u, v, nrm / nn


def _pack(O, u, v, w):
    return np.ascontiguousarray(np.concatenate([O, u, v, w], axis=1))


def table(cls):
    """(records [N] of dtype REC, ouvw [N, 12], P [N, 3])"""
    if cls in _CACHE:
        return _CACHE[cls]
    rng = np.random.default_rng(1000 + CLASSES.index(cls))
    n = N
    size = SIZES[rng.integers(0, len(SIZES), n)]
    wrap = rng.integers(0, 4, n).astype(np.uint32)
    off = rng.integers(0, 1 << 20, n).astype(np.uint32)
    uv = rng.uniform(0, 1, (n, 6))
    O, u, v, w = _frame(rng, n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    if cls == "triangle":
        fold = a + b > 1.0
        a[fold], b[fold] = 1.0 - a[fold], 1.0 - b[fold]
    elif cls == "parallelogram":                           # both sides of the diagonal (gamma < 0 past it), and a little outside
        a, b = rng.uniform(-0.05, 1.05, n), rng.uniform(-0.05, 1.05, n)
    elif cls == "integer_edges":
        # the unit frame at the origin: alpha = P.x and beta = P.y exactly, and with (s, t) = (0,0), (1,0), (0,1) s = alpha, t = beta
        O[:], u[:], v[:], w[:] = 0.0, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
        uv[:] = (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)
        tiny = np.array([-5e-324, 5e-324, -1e-300, -2.0 ** -60, -2.0 ** -53, -2.0 ** -54, 2.0 ** -53, -0.0, 0.0])

        def near(count):
            x = rng.integers(-4, 5, count).astype(np.float64)
            kind = rng.integers(0, 4, count)
            steps = rng.integers(1, 4, count)
            for s in range(1, 4):
                up, dn = (kind == 1) & (steps >= s), (kind == 2) & (steps >= s)
                x[up] = np.nextafter(x[up], np.inf)
                x[dn] = np.nextafter(x[dn], -np.inf)
            t = kind == 3
            x[t] = tiny[rng.integers(0, len(tiny), int(t.sum()))]
            return x
        # (s W and (1 - t) H land on texel borders too: multiples of 1 / W and 1 / H, a few ulps either side)
        a, b = near(n), near(n)
        frac = rng.integers(0, 2, n) == 1
        a[frac] = a[frac] + rng.integers(0, 9, int(frac.sum())) / size[frac, 0].astype(np.float64)
        b[frac] = b[frac] + rng.integers(0, 5, int(frac.sum())) / size[frac, 1].astype(np.float64)
    elif cls == "tiling":
        uv = rng.uniform(-7, 7, (n, 6))
    elif cls == "clamp_far":
        wrap[:] = rng.choice(np.array([1, 2, 3], np.uint32), n)
        uv = rng.uniform(-1, 1, (n, 6)) * 10.0 ** rng.uniform(0, 300, (n, 1))
        a, b = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    elif cls == "needles":
        O, u, v, w = _frame(rng, n, skew=10.0 ** rng.uniform(-9, -2, (n, 1)))
        uv = rng.uniform(-2, 2, (n, 6))
    elif cls == "one_texel":
        size = np.array([(1, 1), (1, 4), (8, 1), (1, 1000), (5, 1)], np.uint32)[rng.integers(0, 5, n)]
        uv = rng.uniform(-2, 2, (n, 6))
    P = O + u * a[:, None] + v * b[:, None]
    if cls == "integer_edges":
        P = np.stack([a, b, np.zeros(n)], axis=1)          # (exactly: no rounding between the table and alpha, beta)
    if cls == "non_finite":
        bad = np.array([np.nan, np.inf, -np.inf, 1e308, -1e308])
        rows = np.arange(n)
        P[rows, rng.integers(0, 3, n)] = bad[rng.integers(0, len(bad), n)]
        both = rng.integers(0, 3, n) == 0
        P[both, 0] = np.nan
    rec = records(size[:, 0], size[:, 1], wrap, uv, off)
    assert rec.dtype == REC
    _CACHE[cls] = (rec, _pack(O, u, v, w), np.ascontiguousarray(P))
    return _CACHE[cls]
