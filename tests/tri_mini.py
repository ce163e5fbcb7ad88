"""The restatement of triangles, written from the contract's text (the header comment of csrc/common/rt_quad.h, include/rt_abi.h
at rt_hip_scene_create_quads, the issue that set it) and not from the kernel.

TEST INFRASTRUCTURE.  A flat primitive is Q, u, v plus a shape; each has a limit lim, 2.0 for a parallelogram and 1.0 for a triangle, and a
hit is accepted iff 0 <= alpha <= 1, 0 <= beta <= 1 and alpha + beta <= lim, the sum one IEEE f64 addition.  Everything else — the constants
(QuadConsts), the steps up to alpha and beta, the record (quad_record), order, ids and ties — is tests/quad_mini.py's.  Plain Python floats,
as there: CPython never fuses a * b + c.
"""
import quad_mini as QM
import mini_oracle as M

SHAPE_PARALLELOGRAM, SHAPE_TRIANGLE = 0, 1
LIM = {SHAPE_PARALLELOGRAM: 2.0, SHAPE_TRIANGLE: 1.0}


def flat_test(c, lim, o, d, closest):
    """the contract's test of one segment against one flat primitive of limit lim: None, or (t, P) of the accepted hit"""
    den = QM.dot(c.N, d)
    if abs(den) < QM.DEN_MIN:
        return None
    num = c.D - QM.dot(c.N, o)
    if den == 0.0:                       # (unreachable, as in quad_test)
        return None
    t = num / den
    if not (t > QM.T_MIN and t < closest):
        return None
    P = (o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)
    p = (P[0] - c.Q[0], P[1] - c.Q[1], P[2] - c.Q[2])
    alpha = QM.dot(c.w, QM.cross(p, c.v))
    beta = QM.dot(c.w, QM.cross(c.u, p))
    if not (0.0 <= alpha and alpha <= 1.0 and 0.0 <= beta and beta <= 1.0):
        return None
    s = alpha + beta
    if not (s <= lim):
        return None
    return t, P


def tri_from_corners(a, b, c):
    """{"triangle": [a, b, c]}: Q = a, u = b - a, v = c - a, one subtraction per component"""
    a, b, c = (tuple(float(x) for x in p) for p in (a, b, c))
    return a, tuple(b[k] - a[k] for k in range(3)), tuple(c[k] - a[k] for k in range(3))


def mesh_triangles(vertices, faces):
    """{"mesh": ...}: its triangles (Q, u, v) in face order"""
    return [tri_from_corners(vertices[i], vertices[j], vertices[k]) for i, j, k in faces]


class TriMini(QM.QuadMini):
    """QuadMini whose entries carry a shape (RtQuad.reserved): hit_world with the limit"""

    def __init__(self, scene, atan2, center1=None, lens=None, quads=None):
        super().__init__(scene, atan2, center1, lens, quads)
        self.lim = [LIM[int(q.reserved)] for q in self.quads]

    def hit_world(self, o, d, node=0):
        hit = QM.SM.SolidMini.hit_world(self, o, d, node)    # every sphere first, in object order
        closest = self.last_t if hit is not None else M.F64_MAX
        best = None
        for k, c in enumerate(self.qc):                      # then entry k before entry k + 1, strict, whatever the shapes
            r = flat_test(c, self.lim[k], o, d, closest)
            if r is not None:
                closest, best = r[0], (k, r[1])
        if best is None:
            return hit
        k, P = best
        self.last_t = closest
        front, normal = QM.quad_record(self.qc[k], d)
        return self.n_spheres + k, P, normal, front
