"""The restatement of what the shutter probe computes, written from the contract's text — csrc/common/rt_quad.h (the list:
the smallest (t, index); a sphere beats a flat entry on an equal t, an earlier entry a later one), rt_flat_motion.h (the entry at tau),
rt_flat_normal.h (the shading normal on the frame at tau) — out of the restatements each of them already has: flat_motion_mini.ConstsAt,
tri_mini.flat_test, smooth_mini.shade, quad_mini.quad_record.  TEST INFRASTRUCTURE.  Plain Python floats: CPython never fuses a * b + c.

The hit a ray already holds takes part in the order like any other: a flat entry held gives way to an entry of a SMALLER index on an equal
t and to nothing else on an equal t; a sphere or a miss gives way only to a smaller t."""
import math

import numpy as np

import flat_motion_mini as MM
import quad_mini as QM
import smooth_mini as SMM
import tri_mini as TM


class World:
    """the per-entry constants of a world of tests/flat_shutter_rays.py, prepared once"""

    def __init__(self, w, id_base, move="world", normals="world"):
        move = w["move"] if isinstance(move, str) else move
        normals = w["normals"] if isinstance(normals, str) else normals
        self.id_base = id_base
        self.c = [QM.QuadConsts(q[0:3], q[3:6], q[6:9]) for q in w["quvs"].tolist()]
        assert all(c.ok for c in self.c)
        self.lim = [TM.LIM[int(s)] for s in w["shapes"]]
        self.mrec = self.nrec = None
        if move is not None:
            made = [MM.prepare(c, m) for c, m in zip(self.c, move.tolist())]
            assert all(kind != MM.BAD for kind, _ in made)
            if any(kind == MM.MOVING for kind, _ in made):       # all zeros: the scene is one that never had any
                self.mrec = [rec for _, rec in made]
        if normals is not None:
            made = [SMM.prepare(n9) for n9 in normals.tolist()]
            assert all(kind != SMM.BAD for kind, _ in made)
            if any(kind == SMM.SMOOTH for kind, _ in made):
                self.nrec = [rec for _, rec in made]

    def at(self, k, tau):
        return MM.ConstsAt(self.c[k], self.mrec[k], tau) if self.mrec is not None else self.c[k]

    def ray(self, o, d, tau, closest, best_in):
        """(best, None) or (best, (t, P, normal, front, origin)) of a newly accepted flat entry: every entry in entry order"""
        best, got = best_in, None
        for k in range(len(self.c)):
            at = self.at(k, tau)
            r = TM.flat_test(at, self.lim[k], o, d, closest)
            if r is None and best >= self.id_base and best - self.id_base > k:      # an equal t: the smaller index takes it
                r = TM.flat_test(at, self.lim[k], o, d, math.nextafter(closest, math.inf))
                if r is not None and r[0] != closest:
                    r = None
            if r is not None:
                closest, best, got = r[0], self.id_base + k, (k, at, r[1])
        if got is None or best == best_in:
            return best, None
        k, at, P = got
        front, normal = QM.quad_record(at, d)
        if self.nrec is not None:
            normal, _ = SMM.shade(at, self.nrec[k], d, P)
        return best, (closest, P, normal, front, at.Q)


def restate(w, rows, id_base, out, move="world", normals="world"):
    """the rays `rows` of a world through World.ray, written into `out` (the dict of arrays of flat_shutter_rays.sentinels) as the probe
    writes them: best always, the rest for a newly accepted flat entry"""
    W = World(w, id_base, move, normals)
    rays, tau, closest = w["rays"][rows].tolist(), w["tau"][rows].astype(np.float64).tolist(), w["closest"][rows].tolist()
    held = w["best_in"][rows].tolist() if w["best_in"] is not None else [-1] * len(rows)
    for j, i in enumerate(rows):
        best, s = W.ray(tuple(rays[j][0:3]), tuple(rays[j][3:6]), tau[j], closest[j], held[j])
        out["best"][i] = best
        if s is not None:
            out["t"][i], out["P"][i], out["normal"][i], out["front"][i], out["origin"][i] = s[0], s[1], s[2], int(s[3]), s[4]
    return out
