"""The restatement of flat primitives that move while the shutter is open, written from the contract's text (the header
comment of csrc/common/rt_flat_motion.h, include/rt_abi.h at rt_hip_scene_set_flat_motion, the issue that set it) and not from the kernel.

TEST INFRASTRUCTURE.  An entry may carry a displacement m over the open shutter; at shutter time tau it is the same primitive translated
by m tau.  Once per entry: the record {m0, m1, m2, Dm}, Dm = dot(N, m); an entry whose three components are all zero stores -0.0 in all
four slots.  Per segment:
    Dtau = D + Dm tau      Qtau_k = q_k + m_k tau      den = dot(N, d)      t = (Dtau - dot(N, o)) / den
    the accept rules of tests/tri_mini.py      P = o + d t      p = P - Qtau      alpha, beta, the limit, front_face, the normal as there
and everything that uses q as a frame — a solid pattern's centre, the weights of the shading normals (tests/smooth_mini.py) — uses Qtau.
tau is the sample's: a scene whose only movers are flat primitives draws it too, its spheres at their own bits.
Plain Python floats: CPython never fuses a * b + c.
"""
import math

import quad_mini as QM
import smooth_mini as SMM
import tri_mini as TM

STILL, MOVING, BAD = 0, 1, 2
STILL_REC = (-0.0, -0.0, -0.0, -0.0)


def _finite(x):
    return x == x and abs(x) != math.inf


def prepare(c, m):
    """(kind, record) of the entry of constants c with displacement m"""
    m = tuple(float(x) for x in m)
    for k in range(3):
        if not _finite(m[k]) or not _finite(c.Q[k] + m[k]):
            return BAD, None
    if m[0] == 0.0 and m[1] == 0.0 and m[2] == 0.0:
        return STILL, STILL_REC
    return MOVING, (m[0], m[1], m[2], QM.dot(c.N, m))


class ConstsAt:
    """the constants of an entry at shutter time tau: Q and D move, u, v, N and w are the entry's"""

    def __init__(self, c, rec, tau):
        self.u, self.v, self.N, self.w, self.ok = c.u, c.v, c.N, c.w, c.ok
        self.Q = (c.Q[0] + rec[0] * tau, c.Q[1] + rec[1] * tau, c.Q[2] + rec[2] * tau)
        self.D = c.D + rec[3] * tau


def moving_test(c, lim, rec, tau, o, d, closest):
    """the contract's test of one segment against one entry at shutter time tau: None, or (t, P, front, normal)"""
    at = ConstsAt(c, rec, tau)
    r = TM.flat_test(at, lim, o, d, closest)
    if r is None:
        return None
    front, normal = QM.quad_record(at, d)
    return r[0], r[1], front, normal


class FlatMotionMini(SMM.SmoothMini):
    """SmoothMini whose entries may move within the frame (move: [n_quads][3] as given, or None)"""

    def __init__(self, scene, atan2, center1=None, lens=None, quads=None, normals=None, move=None):
        super().__init__(scene, atan2, center1, lens, quads, normals)
        self.qc0 = list(self.qc)
        self.mrec = None
        if move is not None:
            assert len(move) == len(self.quads)
            made = [prepare(c, m) for c, m in zip(self.qc0, move)]
            assert all(kind != BAD for kind, _ in made)
            if any(kind == MOVING for kind, _ in made):        # all zeros: the scene is one that never had any
                self.mrec = [rec for _, rec in made]
        if self.mrec is not None and self.dv is None:          # the sample draws its tau; every sphere keeps its bits (dv = -0.0)
            self.dv = [(-0.0, -0.0, -0.0) for _ in self.c0]

    def set_tau(self, tau):
        super().set_tau(tau)
        if self.mrec is not None:
            self.qc = [ConstsAt(c, rec, tau) for c, rec in zip(self.qc0, self.mrec)]
