"""TEST INFRASTRUCTURE: cameras and crafted buffers for the temporal reprojection tests (tests/test_temporal_cpu.py on the CPU build of
reproject_pixel, tests/test_temporal_gpu.py on rt_hip_reproject), each compared with tests/temporal_ref.py bit for bit."""
import math

import numpy as np

F = np.float32


def camera(look_from, look_at, vup=(0.0, 1.0, 0.0), vfov=20.0, aspect=1.5):
    """the four vectors of camera.rs:45-77 as the 12 doubles rt_hip_reproject takes: origin, lower_left, horizontal, vertical"""
    lf, la, up = (np.asarray(v, np.float64) for v in (look_from, look_at, vup))
    vh = 2.0 * math.tan(math.radians(vfov) / 2.0)
    vw = aspect * vh
    w = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    hor, ver = u * vw, v * vh
    ll = lf - hor / 2.0 - ver / 2.0 - w
    return np.concatenate([lf, ll, hor, ver])


def orbit(look_from, look_at, deg):
    """look_from turned about the y axis around look_at"""
    lf, la = np.asarray(look_from, np.float64), np.asarray(look_at, np.float64)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    d = lf - la
    return la + np.array([d[0] * c + d[2] * s, d[1], -d[0] * s + d[2] * c])


LOOK_FROM, LOOK_AT = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0)


def camera_pairs():
    """name -> (current camera, previous camera)"""
    lf, la = np.array(LOOK_FROM), np.array(LOOK_AT)
    cur = camera(lf, la)
    return {
        "identical": (cur, cur.copy()),
        "orbit3": (cur, camera(orbit(lf, la, -3.0), la)),
        "orbit90": (cur, camera(orbit(lf, la, -90.0), la)),
        "behind": (cur, camera(lf, 2.0 * lf - la)),                    # the previous camera looks the other way: a < 0 everywhere
        "through": (cur, camera(lf + 0.9 * (la - lf), la)),            # ... stands in the middle of the scene: some points behind it
    }


def crafted(rng, h, w):
    """(lin, aov, prev_hist, prev_aov): guides constant over 4 x 4 blocks (so that taps find equal and unequal neighbours), depths around
    the camera's distance to look_at, sky pixels (coverage 0), partial coverage, NaN colours in both frames, n' = 0 and NaN n'"""
    by, bx = (np.arange(h) // 4)[:, None], (np.arange(w) // 4)[None, :]
    nb = (h // 4 + 1, w // 4 + 1)
    alb_b = rng.random(nb + (3,)).astype(F)
    nrm_b = rng.normal(size=nb + (3,))
    nrm_b = (nrm_b / np.linalg.norm(nrm_b, axis=-1, keepdims=True)).astype(F)
    t_b = 8.0 + 10.0 * rng.random(nb)
    aov = np.zeros((h, w, 8), F)
    aov[..., 0:3] = alb_b[by, bx]
    aov[..., 4:7] = nrm_b[by, bx]
    cov = np.ones((h, w))
    cov[rng.random((h, w)) < 0.15] = 0.5                      # partial coverage: an edge pixel
    aov[..., 7] = cov
    aov[..., 3] = cov / t_b[by, bx]
    sky = rng.random(nb)[by, bx] < 0.2                        # zero coverage: no normal, no depth
    aov[sky, 3:8] = 0.0
    prev_aov = aov.copy()
    jitter = rng.random((h, w)) < 0.5                         # half the previous frame's pixels differ a little in every guide
    prev_aov[..., 0:3] += (jitter[..., None] * 0.05 * rng.random((h, w, 3))).astype(F)
    prev_aov[..., 4:7] += (jitter[..., None] * 0.05 * rng.random((h, w, 3))).astype(F)
    prev_aov[..., 3] *= (1.0 + jitter * 0.2 * (rng.random((h, w)) - 0.5)).astype(F)
    prev_aov[sky, 3:8] = 0.0
    lin = rng.random((h, w, 3)).astype(F)
    prev_hist = np.zeros((h, w, 4), F)
    prev_hist[..., 0:3] = rng.random((h, w, 3))
    prev_hist[..., 3] = rng.integers(0, 9, (h, w))           # n' = 0: never reused
    for _ in range(h * w // 40 + (h * w > 4)):
        lin[rng.integers(h), rng.integers(w), rng.integers(3)] = np.nan
        prev_hist[rng.integers(h), rng.integers(w), rng.integers(3)] = np.nan
    if h * w > 4:
        prev_hist[rng.integers(h), rng.integers(w), 3] = np.nan
    return lin, aov, prev_hist, prev_aov


# alpha_min, n_max, tau_n, tau_a, tau_z: thresholds 0 and huge, alpha_min 0 and 1, a small and an unbounded n_max
PARAMS = [(0.0, 1e30, 1e30, 1e30, 1e30), (1.0, 4.0, 1e30, 1e30, 1e30), (0.2, 3.0, 0.5, 0.5, 0.5), (0.0, float("inf"), 0.0, 0.0, 0.0),
          (0.1, 32.0, 0.001, 0.001, 0.05)]
SIZES = [(13, 17), (32, 48), (9, 1), (1, 9), (1, 1)]
