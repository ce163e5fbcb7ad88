"""The worlds of the device build of the flat-primitive BVH's order table, shared by the CPU and the GPU tests, and the
builder restated in Python from the issue's contract (not from the C++): centres 0.5 lo + 0.5 hi of the padded boxes, the axis moved only
by a strictly longer extent, the left half the (b - a) / 2 smallest under (centre, index) with the centres compared as doubles, a range
of at most 4 entries a leaf in index order, refused entries in entry order in front.  Every world is triangles (shape 1)."""
import functools

import numpy as np

import flat_update_ref as U

SIZES = (1, 4, 5, 8, 9, 1025, 4099)
SMALL = ("n5", "n8", "n9", "equal", "zeros", "axes", "needles1", "needles4", "needles5")
NEEDLES = {"needles1": [3], "needles4": [3, 9, 20, 30], "needles5": [3, 9, 20, 30, 31]}


def _triangles(rng, n):
    q = rng.uniform(-4.0, 4.0, (n, 3))
    q[:, 1] = rng.uniform(0.0, 1.5, n)
    u = rng.uniform(0.15, 0.6, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    w = rng.uniform(0.15, 0.6, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    v = np.cross(u, w) + 0.25 * w          # never along u
    return np.concatenate([q, u, v], axis=1)


@functools.lru_cache(maxsize=None)
def world(name):
    """quv rows (n x 9), read only"""
    if name[0] == "n" and name[1:].isdigit():
        quv = _triangles(np.random.default_rng(2600 + int(name[1:])), int(name[1:]))
    elif name == "equal":                   # 37 copies of one triangle: every centre equal, every split decided by the index alone
        quv = np.tile([[0.5, 0.2, -1.0, 1.5, 0.0, 0.25, 0.0, 1.0, 0.5]], (37, 1))
    elif name == "zeros":                   # one triangle, its box symmetric about x = 0 (centre exactly +0.0), a third of the copies a hair
        quv = np.tile([[-0.5, 0.2, -1.0, 1.0, 0.0, 0.25, 0.25, 1.0, 0.5]], (41, 1))   # to either side: every split runs along x, ties at 0.0
        quv[1::3, 0] += 2.0 ** -40          # (a padded box never has a centre of -0.0: 0.5 lo + 0.5 hi is -0.0 only for lo = hi = -0.0;
        quv[2::3, 0] -= 2.0 ** -40          #  the CPU test feeds such boxes to the split directly)
    elif name == "axes":                    # four clusters along x, drawn out along x, y, z and x: depth 2 splits along all three axes
        rows = []
        for c, axis in enumerate((0, 1, 2, 0)):
            for k in range(8):
                q = np.array([100.0 * c, 0.0, 0.0])
                q[axis] += 10.0 * k / 7.0
                rows.append(np.concatenate([q, [0.25, 0.0, 0.0], [0.0, 0.25, 0.125]]))
        quv = np.array(rows)[np.random.default_rng(5).permutation(32)]
    elif name in NEEDLES:                   # refused entries: the always-visited run is 1, 4 and 5 entries long
        quv = _triangles(np.random.default_rng(41), 37)
        for k in NEEDLES[name]:
            quv = U.needle(quv, k)
    elif name == "big":                     # 2^16 + 3 triangles of a heightfield: ranges over many workgroups, 15 depths
        from test_flat_bvh_cpu import heightfield
        quv = heightfield(n=182, size=8.0, seed=11)[np.random.default_rng(12).permutation(2 * 182 * 182)[:65539]]
    else:
        raise KeyError(name)
    quv = np.ascontiguousarray(quv, np.float64)
    quv.setflags(write=False)
    return quv


def depths(m):
    """the depths that have a range above 4 entries"""
    d, s = 0, m
    while s > 4:
        d, s = d + 1, (s + 1) // 2
    return d


def python_order(ok, lo, hi, axes=None):
    """the order table of the contract; axes: a dict depth -> set of axes, filled in"""
    ok = np.asarray(ok, bool)
    c = 0.5 * np.asarray(lo, np.float64) + 0.5 * np.asarray(hi, np.float64)
    out = [int(k) for k in np.flatnonzero(~ok)]

    def node(idx, depth):
        if len(idx) <= 4:
            out.extend(sorted(int(k) for k in idx))
            return
        clo, chi = c[idx].min(axis=0), c[idx].max(axis=0)
        axis = 0
        for k in (1, 2):
            if chi[k] - clo[k] > chi[axis] - clo[axis]:
                axis = k
        if axes is not None:
            axes.setdefault(depth, set()).add(axis)
        # (centre, index): Python compares the floats by value, -0.0 == 0.0, then the index
        by = sorted((float(c[k, axis]), int(k)) for k in idx)
        half = len(idx) // 2
        node(np.array(sorted(k for _, k in by[:half])), depth + 1)
        node(np.array(sorted(k for _, k in by[half:])), depth + 1)

    node(np.flatnonzero(ok), 0)
    return np.array(out, np.uint32)
