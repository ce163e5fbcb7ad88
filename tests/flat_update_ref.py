"""Moving the flat primitives of a resident scene: the worlds, the moves and the references the CPU and the GPU tests share.
The refit reference is plain numpy: a node's box is the min / max over the padded boxes (rt_flat_build.h flat_entry_box, through the host
build of tests/flat_bvh_sim.py) of the entries of its subtree, order[first of its first leaf .. first of node `skip`)."""
import functools
import hashlib

import numpy as np

import flat_bvh_sim as F

MOVES = ("translate", "ripple", "scramble")


@functools.lru_cache(maxsize=None)
def world(name):
    """quv rows of the 2 048-triangle heightfield ("2048") or of its 1 025-entry subset ("1025"), read only"""
    from test_flat_bvh_cpu import heightfield
    quv = heightfield()
    if name == "1025":
        quv = quv[np.random.default_rng(31).permutation(2048)[:1025]]
    quv.setflags(write=False)
    return quv


def _corners(quv):
    q, u, v = quv[:, :3], quv[:, 3:6], quv[:, 6:]
    return q.copy(), q + u, q + v


def _from_corners(p0, p1, p2):
    return np.ascontiguousarray(np.concatenate([p0, p1 - p0, p2 - p0], axis=1))


def moved(quv, move, step=1):
    """the world after `move` (MOVES), step 1, 2, ...: n x 9 rows again, every entry still a proper triangle"""
    p = _corners(np.asarray(quv, np.float64))
    s = float(step)
    if move == "translate":          # rigid
        d = np.array([0.75, 0.125, -0.5]) * s
        return _from_corners(*(c + d for c in p))
    if move == "ripple":             # per vertex, by position: a shared vertex stays shared
        def f(c):
            c = c.copy()
            c[:, 1] += 0.35 * np.sin(1.7 * c[:, 0] + s) * np.cos(1.3 * c[:, 2] - 0.5 * s)
            return c
        return _from_corners(*(f(c) for c in p))
    if move == "scramble":           # entry k goes where entry perm[k] was: the entries of a leaf end up far apart
        rng = np.random.default_rng(900 + step)
        perm = rng.permutation(len(quv))
        d = p[0][perm] - p[0]
        d[:, 1] += rng.uniform(0.0, 0.4, len(quv))
        return _from_corners(*(c + d for c in p))
    raise KeyError(move)


def needle(quv, k):
    """entry k stretched into a needle with K = (|u| + |v|)^2 / |cross(u, v)| above 2^20: flat_entry_box refuses it"""
    out = np.array(quv, np.float64)
    out[k, 3:6] = [3000.0, 0.0, 0.0]
    out[k, 6:9] = [0.0, 1e-3, 0.0]
    return out


def refit_reference(sim, flats, nodes, order):
    """the boxes a refit must leave in `nodes` (topology and order as given) for the geometry `flats`: lo, hi (n_nodes x 3).  A leaf of refused
    entries keeps its infinite box."""
    ok, lo, hi = sim.entry_boxes(flats)
    nn = len(nodes)
    first, count, skip = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64), nodes["skip"].astype(np.int64)
    leaves = np.flatnonzero(count > 0)
    # entries below node i: order[start(i) : start(skip[i])], start(i) = first of the first leaf at or behind i
    start = np.full(nn + 1, len(order), np.int64)
    start[leaves] = first[leaves]
    for i in range(nn - 1, -1, -1):
        if count[i] == 0:
            start[i] = start[i + 1]
    out_lo, out_hi = np.zeros((nn, 3)), np.zeros((nn, 3))
    for i in range(nn):
        ks = order[start[i]:start[skip[i]]]
        if not ok[ks].all():
            assert count[i] > 0 and not ok[ks].any()
            out_lo[i], out_hi[i] = -np.inf, np.inf
        else:
            out_lo[i], out_hi[i] = lo[ks].min(axis=0), hi[ks].max(axis=0)
    return out_lo, out_hi


def refit_nodes(sim, flats, nodes, order):
    """`nodes` with the reference boxes: what "flat_bvh" must hold, byte for byte, after a refit to `flats`"""
    out = np.array(nodes, F.NODE)
    out["lo"], out["hi"] = refit_reference(sim, flats, nodes, order)
    return out


def digest(*blobs):
    h = hashlib.sha256()
    for b in blobs:
        h.update(len(b).to_bytes(8, "little"))
        h.update(b)
    return h.hexdigest()
