"""The point tables of the solid-texture code's bit tests, shared by the host build's test (tests/test_solid_cpu.py) and the
device's (tests/test_solid_points_gpu.py): six classes of points in the sphere's frame, >= 10^5 each, each aimed at one place where two
builds of csrc/common/rt_solid.h could part ways.  class_points(cls) is the class's table (n x 3 f64, read-only, drawn once per session
from a fixed seed); edge_rows(cls) the rows that carry the class's edge; subset(cls, m) those rows and a stride through the rest.  Every
class runs over SEEDS and over MODES (class_modes(cls): octave_overflow adds 8 octaves).

  mixed            the table of tests/test_solid_cpu.py since the solid textures came: mixed(rng, n), unchanged
  tiny_negative    -2^-k, k = 1 .. 1074, on one axis or on all three: floor is -1 and p - floor(p) rounds to exactly 1.0 from k = 54 on
  octave_overflow  one coordinate at +-2^(31 - j) and its two neighbours, j = 0 .. 16: octave j of a turbulence is the first outside the
                   lattice's range (rt_solid_noise returns 0.0 there), or one ulp inside it
  int32_wrap       floor(p_c) at the ends of the int32 range: (uint32)(int32)(int64) of it, and i + 1 wrapping to 0x80000000
  lattice_marble   N = T = 0 exactly (whole coordinates, or -2^-k, k >= 70, on z), so marble's phase is INV_2PI * p_z alone: x - floor(x) is 0, just
                   below 1.0, or rounds to 1.0
  checker_planes   pairs one ulp either side of a whole number of every magnitude up to 2^52 and beyond"""
import functools
from fractions import Fraction

import numpy as np

import solid_mini as SM

SEEDS = (0, 0xFFFFFFFF, 0x9E3779B9)
MODES = [(SM.MODE_NOISE, 7), (SM.MODE_TURBULENCE, 1), (SM.MODE_TURBULENCE, 16), (SM.MODE_MARBLE, 1), (SM.MODE_MARBLE, 16)]
CLASSES = ["mixed", "tiny_negative", "octave_overflow", "int32_wrap", "lattice_marble", "checker_planes"]
N = 105_000
INV_2PI = 0.15915494309189535
TWO31, TWO52 = 2.0 ** 31, 2.0 ** 52


def class_modes(cls):
    return MODES + ([(SM.MODE_TURBULENCE, 8)] if cls == "octave_overflow" else [])


def mixed(rng, n):
    """n points: mostly a few cells around the origin (negative coordinates included), some on lattice planes (t_c = 0), some of every
    magnitude, some around +-2^31 and +-2^52, some non-finite"""
    p = rng.uniform(-40.0, 40.0, (n, 3))
    k = n // 10
    p[:k] = np.round(p[:k]) + rng.uniform(0.0, 1.0, (k, 3)) * (rng.random((k, 3)) < 0.5)                 # whole coordinates
    p[k:2 * k] = rng.standard_normal((k, 3)) * 10.0 ** rng.uniform(-8, 12, (k, 1))                      # every magnitude
    edge = np.array([2.0 ** 31, -2.0 ** 31, np.nextafter(2.0 ** 31, 0.0), -np.nextafter(2.0 ** 31, 0.0), np.nextafter(2.0 ** 31, np.inf),
                     2.0 ** 31 - 0.5, -2.0 ** 31 + 0.5, 2.0 ** 30, 2.0 ** 52, -2.0 ** 52, np.nextafter(2.0 ** 52, 0.0), -np.nextafter(2.0 ** 52, 0.0),
                     2.0 ** 52 - 1.0, 2.0 ** 52 + 2.0, 2.0 ** 53, -2.0 ** 63, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-310, -1e-310, -1.0, 1.0, 0.5])
    m = 2 * k
    sel = rng.integers(0, len(edge), (k, 3))
    p[m:m + k] = np.where(rng.random((k, 3)) < 0.4, edge[sel], p[m:m + k])
    for j, e in enumerate(edge):                        # every edge value on every axis at least once
        for c in range(3):
            p[m + k + 3 * j + c, c] = e
    return p


# ------------------------------------------------------------------ tiny_negative
TINY_ROUND = 4 * 1074          # k = 1 .. 1074 on axis 0, 1, 2 and on all three
TINY_ROUNDS = 25


def tiny_k():
    """the k of every row of tiny_negative: even rounds run k = 1 .. 1074, odd rounds stay at k = 1 .. 53, where p - floor(p) is below 1.0"""
    full = np.arange(1, 1075)
    return np.concatenate([np.tile(full if r % 2 == 0 else 1 + (full - 1) % 53, 4) for r in range(TINY_ROUNDS)])


def tiny_axes():
    """which axes of a row hold -2^-k (n x 3 bool)"""
    one = np.zeros((TINY_ROUND, 3), bool)
    for c in range(3):
        one[c * 1074:(c + 1) * 1074, c] = True
    one[3 * 1074:] = True
    return np.tile(one, (TINY_ROUNDS, 1))


def _tiny_negative(rng):
    p = rng.uniform(-40.0, 40.0, (TINY_ROUND * TINY_ROUNDS, 3))
    v = -np.ldexp(1.0, -tiny_k())
    return np.where(tiny_axes(), v[:, None], p)


# ------------------------------------------------------------------ octave_overflow
OCT_ROUND = 17 * 2 * 3 * 3     # j, sign, {one ulp inside, at, one ulp outside}, axis
OCT_ROUNDS = 344


def octave_layout():
    """per row of one round: j, sign, side (-1: one ulp inside, 0: at 2^(31 - j), +1: one ulp outside), axis"""
    j, sign, side, axis = np.meshgrid(np.arange(17), [1.0, -1.0], [-1, 0, 1], np.arange(3), indexing="ij")
    return j.reshape(-1), sign.reshape(-1), side.reshape(-1), axis.reshape(-1)


def _octave_overflow(rng):
    j, sign, side, axis = (np.tile(a, OCT_ROUNDS) for a in octave_layout())
    p = rng.uniform(-40.0, 40.0, (OCT_ROUND * OCT_ROUNDS, 3))
    at = np.ldexp(1.0, 31 - j)
    v = sign * np.where(side < 0, np.nextafter(at, 0.0), np.where(side > 0, np.nextafter(at, np.inf), at))
    p[np.arange(len(p)), axis] = v
    return p


# ------------------------------------------------------------------ int32_wrap
WRAP_FLOORS = np.array([-TWO31, -TWO31 + 1.0, TWO31 - 2.0, TWO31 - 1.0])
WRAP_FRACS = np.array([0.0, 0.5, 1.0 - 2.0 ** -22])


def _int32_wrap(rng):
    """every (floor, fraction) on every axis alone in the first 36 rows; then 1 .. 3 axes of a row at such values, the rest generic.  floor +
    fraction is exact: 31 bits before the point and 22 behind it"""
    p = rng.uniform(-40.0, 40.0, (N, 3))
    special = rng.random((N, 3)) < 0.5
    special[np.arange(N), rng.integers(0, 3, N)] = True
    v = WRAP_FLOORS[rng.integers(0, 4, (N, 3))] + WRAP_FRACS[rng.integers(0, 3, (N, 3))]
    p = np.where(special, v, p)
    r = 0
    for c in range(3):
        for f in WRAP_FLOORS:
            for t in WRAP_FRACS:
                p[r] = rng.uniform(-40.0, 40.0, 3)
                p[r, c] = f + t
                r += 1
    return p


# ------------------------------------------------------------------ lattice_marble
def near_whole_phases():
    """whole p_z, |p_z| < 2^53, for which the double INV_2PI * p_z lies within 4 ulps of a whole number without being one, and has at least
    20 bits behind the point: multiples of the denominators of INV_2PI's continued fraction, found here by trying them"""
    c = Fraction(INV_2PI)
    h0, h1, k0, k1 = 0, 1, 1, 0
    dens = []
    x = c
    for _ in range(40):
        a = x.numerator // x.denominator
        h0, h1, k0, k1 = h1, a * h1 + h0, k1, a * k1 + k0
        dens.append(k1)
        if x == a:
            break
        x = 1 / (x - a)
    cand = np.array(sorted({float(s * m * d) for d in dens if 2 ** 8 <= d < 2 ** 34 for m in range(1, 257) if m * d < 2 ** 34 for s in (1, -1)}))
    ph = INV_2PI * cand
    off = np.abs(ph - np.rint(ph))
    keep = (off > 0.0) & (off <= 4.0 * np.spacing(np.abs(ph))) & (np.abs(ph) < 2.0 ** 31)
    return cand[keep]


def marble_phase(p):
    """marble's x and s = x - floor(x) for a table whose T is 0: x = INV_2PI * (p_z + 10.0 * 0.0)"""
    x = INV_2PI * (p[:, 2] + 10.0 * 0.0)
    return x, x - np.floor(x)


def _lattice_marble(rng):
    near = near_whole_phases()
    assert len(near) >= 8, len(near)
    p = np.rint(rng.uniform(-1000.0, 1000.0, (N, 3)))
    big = rng.random(N) < 0.2
    p[big, :2] = np.rint(rng.uniform(-TWO31 + 1.0, TWO31 - 1.0, (int(big.sum()), 2)))
    z = np.rint(rng.uniform(-TWO31 + 1.0, TWO31 - 1.0, N))
    z = np.where(rng.random(N) < 0.3, np.rint(rng.uniform(-1000.0, 1000.0, N)), z)
    pick = rng.integers(0, 4, N)
    z = np.where(pick == 1, near[rng.integers(0, len(near), N)], z)
    tiny = -np.ldexp(1.0, -rng.integers(70, 1075, N))          # x, y whole and z = -2^-k, k >= 54 + 16: t_z rounds to 1.0 in all 16 octaves, N is 0 still
    z = np.where(pick == 2, tiny, z)
    p[:, 2] = z
    head = np.concatenate([[0.0, -0.0, 1.0, -1.0, TWO31 - 1.0, -(TWO31 - 1.0), -2.0 ** -70, -2.0 ** -1074, -2.0 ** -100], near])
    p[:len(head), 2] = head
    return p


# ------------------------------------------------------------------ checker_planes
PLANE_PAIRS = N // 2
PLANE_BELOW = 31_500           # pairs around whole numbers below 2^52 in magnitude; the rest at and beyond 2^52


def _checker_planes(rng):
    """rows i and PLANE_PAIRS + i are a pair: on one axis, one ulp below the whole number w and w itself; the other axes generic"""
    m = PLANE_PAIRS
    mag = np.floor(2.0 ** rng.uniform(0.0, 52.0, m))
    mag[:53] = 2.0 ** np.arange(53)                              # (w = 2^52 itself: the bound)
    mag[53:106] = 2.0 ** np.arange(53) - 1.0
    mag[PLANE_BELOW:] = TWO52 * np.floor(2.0 ** rng.uniform(0.0, 10.0, m - PLANE_BELOW))
    mag[52] = TWO52
    w = mag * np.where(rng.random(m) < 0.5, 1.0, -1.0)
    base = rng.uniform(-200.0, 200.0, (m, 3))
    axis = rng.integers(0, 3, m)
    lo, hi = base.copy(), base.copy()
    lo[np.arange(m), axis] = np.nextafter(w, -np.inf)
    hi[np.arange(m), axis] = w
    return np.concatenate([lo, hi])


def numpy_parity(p):
    f = np.floor(p)
    ok = (np.abs(f) < TWO52).all(axis=1)
    s = np.where(ok[:, None], f, 0.0).astype(np.int64).sum(axis=1)
    return np.where(ok, s & 1, 0).astype(np.int32)


_DRAW = {"tiny_negative": (_tiny_negative, 1701), "octave_overflow": (_octave_overflow, 1702), "int32_wrap": (_int32_wrap, 1703),
         "lattice_marble": (_lattice_marble, 1704), "checker_planes": (_checker_planes, 1705)}
# the rows that carry each class's edge (always part of a subset): the leading rows, in which every case stands once
_EDGE_ROWS = {"octave_overflow": OCT_ROUND, "int32_wrap": 36, "lattice_marble": 64, "checker_planes": 106}


@functools.lru_cache(maxsize=None)
def class_points(cls):
    if cls == "mixed":
        p = mixed(np.random.default_rng(1616), 100_000)      # (test_noise_and_checker_equal_the_restatement_bit_for_bit's table)
    else:
        fn, seed = _DRAW[cls]
        with np.errstate(all="ignore"):
            p = fn(np.random.default_rng(seed))
    p = np.ascontiguousarray(p, np.float64)
    assert p.shape[1] == 3 and len(p) >= 100_000, (cls, p.shape)
    p.setflags(write=False)
    return p


def edge_rows(cls):
    n = len(class_points(cls))
    if cls == "mixed":                       # the rows `mixed` writes its edge values into
        k = n // 10
        return np.arange(2 * k + k, 2 * k + k + 3 * 26)
    if cls == "checker_planes":              # both halves of the leading pairs
        return np.concatenate([np.arange(106), PLANE_PAIRS + np.arange(106), PLANE_BELOW + np.arange(20), PLANE_PAIRS + PLANE_BELOW + np.arange(20)])
    if cls == "tiny_negative":               # of the first round, the k either side of the switch at 54, the ends, and the normal / subnormal border
        k = tiny_k()[:TINY_ROUND]
        return np.flatnonzero(((k >= 46) & (k <= 62)) | (k <= 2) | ((k >= 1021) & (k <= 1024)) | (k >= 1073))
    return np.arange(_EDGE_ROWS[cls])


def subset(cls, m=2000):
    """>= m rows of the class: the rows that carry its edge, and a stride through the whole table"""
    n = len(class_points(cls))
    return np.unique(np.concatenate([edge_rows(cls), np.arange(0, n, max(1, n // m))]))
