"""Adversarial hit tables for the shading normal of a triangle: per class N points, each its own entry — (quv [N, 9],
vertex normals as given [N, 9], d [N, 3], P [N, 3]).  TEST INFRASTRUCTURE: seeded, computed once, read-only."""
import functools

import numpy as np

N = 100_000
CLASSES = ["generic", "edges", "opposite", "side", "grazing", "needle", "non_finite"]


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _tri(rng, n, needle=False):
    q = rng.uniform(-3, 3, (n, 3))
    u = rng.uniform(-2, 2, (n, 3))
    v = rng.uniform(-2, 2, (n, 3))
    if needle:   # nearly parallel edges, or edges of very different lengths
        half = n // 2
        v[:half] = u[:half] * rng.uniform(0.5, 2.0, (half, 1)) + rng.uniform(-1, 1, (half, 3)) * 10.0 ** rng.uniform(-9, -4, (half, 1))
        u[half:] *= 10.0 ** rng.uniform(-6, -3, (n - half, 1))
        v[half:] *= 10.0 ** rng.uniform(1, 3, (n - half, 1))
    return q, u, v


def _nudge(x, rng, k=3):
    """x moved by up to k ulps"""
    b = np.ascontiguousarray(x, np.float64).view(np.int64) + rng.integers(-k, k + 1, x.shape)
    return b.view(np.float64)


def _gen(cls, rng, ne, rep):
    """ne entries (geometry and vertex normals), rep points on each: (quv, normals, d, P), ne * rep rows, an entry's rows together"""
    n = ne * rep
    R = lambda x: np.repeat(x, rep, axis=0)
    q, u, v = (R(x) for x in _tri(rng, ne, needle=cls == "needle"))
    Ng = _unit(np.cross(u, v))
    a = rng.uniform(0, 1, n); b = rng.uniform(0, 1, n)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    nrm = _unit(Ng[:, None, :] + R(rng.uniform(-0.8, 0.8, (ne, 3, 3)))) * R(rng.uniform(0.2, 5.0, (ne, 3, 1)))   # three normals about N, any length
    d = rng.uniform(-1, 1, (n, 3))
    if cls == "edges":      # alpha, beta, gamma within ulps of 0 and 1
        pick = np.array([0.0, 1.0, 0.5, 1e-17, 1 - 1e-16])
        a = pick[rng.integers(0, 5, n)]
        b = np.where(rng.random(n) < 0.5, 1.0 - a, pick[rng.integers(0, 5, n)] * (1.0 - a))
        a, b = _nudge(a + 0.0, rng), _nudge(b + 0.0, rng)
    if cls == "opposite":   # n0 = -n1 and n2 across: m nearly cancels at gamma = alpha, mm around 1e-24 on both sides
        t = R(_unit(rng.uniform(-1, 1, (ne, 3))))
        nrm[:, 0], nrm[:, 1] = t, -t
        nrm[:, 2] = _unit(np.cross(t, R(rng.uniform(-1, 1, (ne, 3)))))
        b = 10.0 ** rng.uniform(-14, -10, n)
        a = (1.0 - b) / 2.0
    if cls == "side":       # normals in the face's plane plus a few ulps of N either way: dot(s, N) within ulps of 0
        t = _unit(np.cross(Ng, R(rng.uniform(-1, 1, (ne, 3)))))
        eps = R(rng.integers(-4, 5, (ne, 1))) * 2.0 ** -53
        nrm[:, 0] = nrm[:, 1] = nrm[:, 2] = t + eps * Ng
    P = q + a[:, None] * u + b[:, None] * v
    if cls == "grazing":    # d in the plane perpendicular to the interpolated normal, a few ulps either way
        g = 1.0 - a - b
        nu = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
        s = _unit(g[:, None] * nu[:, 0] + a[:, None] * nu[:, 1] + b[:, None] * nu[:, 2])
        t = _unit(np.cross(s, rng.uniform(-1, 1, (n, 3))))
        d = t + rng.integers(-4, 5, (n, 1)) * 2.0 ** -53 * s
    return np.concatenate([q, u, v], axis=1), nrm.reshape(n, 9).copy(), np.ascontiguousarray(d), np.ascontiguousarray(P)


DEVICE_CLASSES = ["generic", "edges", "opposite", "side", "grazing", "needle", "scales"]
DEVICE_ENTRIES, DEVICE_REP = 1000, 103       # 103 000 points per class; 103 rays per launch: one wave and a partial one


@functools.lru_cache(maxsize=None)
def device_table(cls):
    """The classes as the device can be given them (tests/test_smooth_gpu.py, through rt_hip_quad_probe): DEVICE_ENTRIES triangles with
    their normals and DEVICE_REP rays on each — (quv [E, 9], normals [E, 9], rays [E * REP, 6]).  A ray is o = P - d T, d: the device forms P
    itself (o + d t, t ~ T), as every frame does.  "scales" is what of the non_finite class can reach a shaded hit: geometry scaled by
    10^[0, 60], normals by 10^[-140, 140] with subnormal components.  What cannot: a NaN or inf normal is refused by
    rt_hip_scene_set_flat_normals before any kernel sees it; a NaN or inf in o or d fails the hit test (every comparison), so no hit is
    shaded; geometry far below 1 is not hit within t > 0.001 and |dot(N, d)| >= 1e-8 at a P that still resolves the triangle."""
    rng = np.random.default_rng(2600 + DEVICE_CLASSES.index(cls))
    E, rep = DEVICE_ENTRIES, DEVICE_REP
    quv, nr, d, P = _gen("generic" if cls == "scales" else cls, rng, E, rep)
    T = np.ones((E * rep, 1))
    if cls == "scales":
        gs = np.repeat(10.0 ** rng.uniform(0, 60, (E, 1)), rep, axis=0)
        quv, P, T = quv * gs, P * gs, gs
        nr = nr * np.repeat(10.0 ** rng.uniform(-140, 140, (E, 1)), rep, axis=0)
        tiny = np.repeat(rng.random((E, 9)) < 0.1, rep, axis=0)
        nr[tiny] = np.where(np.repeat(rng.random((E, 9)) < 0.5, rep, axis=0)[tiny], 5e-324, -2.5e-310)
    rays = np.concatenate([P - d * T, d], axis=1)
    out = (np.ascontiguousarray(quv[::rep]), np.ascontiguousarray(nr[::rep]), np.ascontiguousarray(rays))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table(cls):
    rng = np.random.default_rng(2500 + CLASSES.index(cls))
    quv, nr, d, P = _gen(cls, rng, N, 1)
    n = N
    if cls == "non_finite":  # NaN, inf, subnormal components and scales over 10^+-150, in every input
        special = np.array([np.nan, np.inf, -np.inf, 5e-324, -2.5e-310, 1e-160, 1e160, -1e200, 0.0, -0.0])
        scale = 10.0 ** rng.uniform(-160, 160, (n, 1))
        k = n // 4
        quv[:k] *= scale[:k]; P[:k] *= scale[:k]
        for arr in (nr[k:2 * k], d[2 * k:3 * k], P[3 * k:]):
            m = rng.random(arr.shape) < 0.25
            arr[m] = special[rng.integers(0, len(special), int(m.sum()))]
        nr[k:2 * k] *= 10.0 ** rng.uniform(-160, 160, (k, 1))
    out = (quv, nr, d, P)
    for x in out:
        x.setflags(write=False)
    return out
