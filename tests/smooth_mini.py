"""The restatement of shading normals on triangles, written from the contract's text (the header comment of
csrc/common/rt_flat_normal.h, include/rt_abi.h at rt_hip_scene_set_flat_normals, the issue that set it) and not from the kernel.

TEST INFRASTRUCTURE.  Per entry three vertex normals n0, n1, n2 at Q, Q + u, Q + v; all nine components zero: the entry shades flat.
Prepared once: n_i / sqrt(dot(n_i, n_i)), three divisions per vector.  Per accepted hit — the test, t, ids and ties are tests/tri_mini.py's:
    p = P - Q    alpha = dot(w, cross(p, v))    beta = dot(w, cross(u, p))    gamma = (1 - alpha) - beta
    m_c = (n0_c gamma + n1_c alpha) + n2_c beta       mm = dot(m, m)      s = m / sqrt(mm)
    not (mm > 1e-24): s = N;  else not (dot(s, N) > 0): s = N
    front = dot(d, N) < 0       normal = s if front else -s
    not (dot(d, normal) < 0): normal = N if front else -N
Plain Python floats: CPython never fuses a * b + c.
"""
import math

import quad_mini as QM
import tri_mini as TM

MM_MIN = 1e-24
FELL_MM, FELL_SIDE, FELL_GRAZING, NO_NORMALS = 1, 2, 4, 8
FLAT, SMOOTH, BAD = 0, 1, 2


def _finite(x):
    return x == x and abs(x) != math.inf


def prepare(n9):
    """(kind, record) of one entry's nine components: FLAT with nine zeros, SMOOTH with three unit vectors, or BAD"""
    n9 = [float(x) for x in n9]
    if all(x == 0.0 for x in n9):
        return FLAT, (0.0,) * 9
    out = []
    for i in range(3):
        n = n9[3 * i:3 * i + 3]
        if not all(_finite(x) for x in n):
            return BAD, None
        nn = QM.dot(n, n)
        if not (_finite(nn) and nn >= 2.2250738585072014e-308):
            return BAD, None
        ln = math.sqrt(nn)
        out += [n[0] / ln, n[1] / ln, n[2] / ln]
    return SMOOTH, tuple(out)


def _div(a, b):
    """IEEE a / b where Python would raise"""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def shade(c, rec, d, P):
    """(normal, fell) of a hit at P by a segment of direction d on the entry of constants c whose prepared record is rec"""
    N = c.N
    front = QM.dot(d, N) < 0.0
    if rec[0] == 0.0 and rec[1] == 0.0 and rec[2] == 0.0:
        return (N if front else (-N[0], -N[1], -N[2])), NO_NORMALS
    p = (P[0] - c.Q[0], P[1] - c.Q[1], P[2] - c.Q[2])
    alpha = QM.dot(c.w, QM.cross(p, c.v))
    beta = QM.dot(c.w, QM.cross(c.u, p))
    gamma = (1.0 - alpha) - beta
    m = tuple((rec[k] * gamma + rec[3 + k] * alpha) + rec[6 + k] * beta for k in range(3))
    mm = QM.dot(m, m)
    ln = math.sqrt(mm) if mm >= 0.0 else math.nan
    s = tuple(_div(m[k], ln) for k in range(3))
    fell = 0
    if not (mm > MM_MIN):
        fell |= FELL_MM
    elif not (QM.dot(s, N) > 0.0):
        fell |= FELL_SIDE
    if fell:
        s = N
    normal = s if front else (-s[0], -s[1], -s[2])
    if not (QM.dot(d, normal) < 0.0):
        fell |= FELL_GRAZING
        normal = N if front else (-N[0], -N[1], -N[2])
    return normal, fell


class SmoothMini(TM.TriMini):
    """TriMini whose entries may carry shading normals ([n_quads][9] as given, or None): the record's normal is the contract's"""

    def __init__(self, scene, atan2, center1=None, lens=None, quads=None, normals=None):
        super().__init__(scene, atan2, center1, lens, quads)
        self.rec = None
        self.fell = {FELL_MM: 0, FELL_SIDE: 0, FELL_GRAZING: 0}
        self.shaded = 0
        if normals is not None:
            assert len(normals) == len(self.quads)
            self.rec = []
            for k, n9 in enumerate(normals):
                kind, rec = prepare(n9)
                assert kind != BAD and (kind == FLAT or self.lim[k] == 1.0), k
                self.rec.append(rec)

    def hit_world(self, o, d, node=0):
        hit = super().hit_world(o, d, node)
        if hit is None or self.rec is None or hit[0] < self.n_spheres:
            return hit
        i, P, _, front = hit
        k = i - self.n_spheres
        normal, fell = shade(self.qc[k], self.rec[k], d, P)
        if not fell & NO_NORMALS:
            self.shaded += 1
            for b in self.fell:
                if fell & b:
                    self.fell[b] += 1
        return i, P, normal, front
