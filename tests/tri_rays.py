"""The ray tables of the triangle bit tests, shared by the host build's test (tests/test_tri_cpu.py) and the device's
(tests/test_tri_gpu.py): the nine classes of tests/quad_rays.py — the same batches, read as triangles (lim = 1) — and a tenth, `hypotenuse`,
aimed at the one comparison a triangle adds: alpha + beta <= 1.

hypotenuse = 50 generic triangles x 1 000 rays aimed at (a, 1 - a + off), off from 1e-17 to 1e-3 on either side (and 0), plus ONE batch of
50 000 rays against HYP_QUV, whose alpha and beta are EXACT functions of the ray: Q = (0, 0, 0.5), u = (4, 0, 0), v = (0, 2, 0) give
N = (0, 0, 1), D = 0.5, w = (0, 0, 1/8); a ray from (4 a, 2 b, 0.5 + s) along (0, 0, -s), s a power of two, has t = 1, P = (4 a, 2 b, 0.5),
alpha = a and beta = b without a rounding.  There a is a multiple of 2^-20 and b is 1 - a moved by -4 .. 4 ulps, so alpha + beta is the one
rounded addition of the contract on either side of 1, and exactly 1 (k = 0: (1/2, 1/2), (1/4, 3/4), ...: accepted)."""
import numpy as np

from quad_rays import CLASSES, N_R, T_MAX, _aimed, _quads, _ulps, class_tables, device_class_tables

TRI_CLASSES = CLASSES + ["hypotenuse"]
HYP_QUV = np.array([0.0, 0.0, 0.5, 4.0, 0.0, 0.0, 0.0, 2.0, 0.0])
N_HYP_Q, N_HYP_EXACT = 50, 50_000


def exact_rays(a, b, rng=None):
    """rays whose (alpha, beta) against HYP_QUV are exactly (a, b) (a, b with at most 50 significant bits below 2): n x 6"""
    n = len(a)
    s = np.ones(n) if rng is None else 2.0 ** rng.integers(-2, 3, n)
    return np.stack([4.0 * a, 2.0 * b, 0.5 + s, np.zeros(n), np.zeros(n), -s], axis=1)


def _hypotenuse():
    rng = np.random.default_rng(2010)
    for quv in _quads(rng, N_HYP_Q, "generic"):
        closest = np.where(rng.random(N_R) < 0.5, T_MAX, rng.uniform(0.0, 8.0, N_R))
        a = rng.uniform(0.0, 1.0, N_R)
        off = 10.0 ** rng.uniform(-17, -3, N_R) * np.where(rng.random(N_R) < 0.5, 1.0, -1.0)
        off[rng.random(N_R) < 0.1] = 0.0
        yield quv, _aimed(rng, quv, N_R, np.stack([a, (1.0 - a) + off], axis=1)), closest
    a = rng.integers(0, 2 ** 20 + 1, N_HYP_EXACT) * 2.0 ** -20
    a[:8] = [0.5, 0.25, 0.75, 0.125, 0.875, 0.0, 1.0, 2.0 ** -20]
    k = rng.integers(-4, 5, N_HYP_EXACT)
    k[:8] = 0
    b = _ulps(1.0 - a, k)
    b = np.where(1.0 - a == 0.0, np.maximum(k, 0) * 2.0 ** -53, b)        # (a = 1: beta = 0 or just above, never negative by an ulp of 0)
    yield HYP_QUV, exact_rays(a, b, rng), np.full(N_HYP_EXACT, T_MAX)


def tri_class_tables(cls):
    """(quv, rays, closest) batches of one class, every quv read as a triangle"""
    if cls == "hypotenuse":
        yield from _hypotenuse()
    else:
        yield from class_tables(cls)


def tri_device_class_tables(cls, sim=None):
    """tri_class_tables(cls) for a device scene (quad_rays.device_class_tables: no refused entry); every hypotenuse entry is accepted as drawn"""
    if cls == "hypotenuse":
        yield from _hypotenuse()
    else:
        yield from device_class_tables(cls, sim)
