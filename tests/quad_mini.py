"""The restatement of quads, written from the contract's text (include/rt_abi.h at rt_hip_scene_create_quads, the header
comment of csrc/common/rt_quad.h, the issue that set it) and not from the kernel.

TEST INFRASTRUCTURE.  QuadMini is tests/solid_mini.py's SolidMini — shutter time, thin lens, media, solids, the discarded count — with
hit_world, the surface record, the first-hit AOVs and scatter's material lookup extended by the scene's quads: quad k is object
n_spheres + k, tested behind every sphere under a strict comparison.  The arithmetic is plain Python floats (CPython never fuses
a * b + c): one IEEE f64 operation per step, in the contract's order.
"""
import math

import numpy as np

import mini_oracle as M
import solid_mini as SM

T_MIN = 0.001
DEN_MIN = 1e-8
SURFACE_NONE = 0xFFFFFFFF


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def _finite(x):
    return x == x and abs(x) != math.inf


class QuadConsts:
    """the per-quad constants of the contract: n = cross(u, v), nn = dot(n, n), len = sqrt(nn), N = n / len, D = dot(N, Q), w = n / nn.
    ok: q, u, v finite and nn neither zero, subnormal nor non-finite"""

    def __init__(self, q, u, v):
        self.Q, self.u, self.v = tuple(map(float, q)), tuple(map(float, u)), tuple(map(float, v))
        self.ok = all(_finite(x) for x in self.Q + self.u + self.v)
        self.N = self.w = (math.nan,) * 3
        self.D = math.nan
        if not self.ok:
            return
        n = cross(self.u, self.v)
        nn = dot(n, n)
        if not (_finite(nn) and nn >= 2.2250738585072014e-308):
            self.ok = False
            return
        ln = math.sqrt(nn)
        self.N = (n[0] / ln, n[1] / ln, n[2] / ln)
        self.D = dot(self.N, self.Q)
        self.w = (n[0] / nn, n[1] / nn, n[2] / nn)


def quad_test(c, o, d, closest):
    """the contract's test of one segment against one quad: None, or (t, P) of the accepted hit"""
    den = dot(c.N, d)
    if abs(den) < DEN_MIN:
        return None
    num = c.D - dot(c.N, o)
    if den == 0.0:                       # (unreachable: |0| < 1e-8; Python would raise where IEEE gives inf or NaN)
        return None
    t = num / den
    if not (t > T_MIN and t < closest):  # (a NaN fails both)
        return None
    P = (o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)
    p = (P[0] - c.Q[0], P[1] - c.Q[1], P[2] - c.Q[2])
    alpha = dot(c.w, cross(p, c.v))
    beta = dot(c.w, cross(c.u, p))
    if not (0.0 <= alpha and alpha <= 1.0 and 0.0 <= beta and beta <= 1.0):
        return None
    return t, P


def quad_record(c, d):
    """(front_face, normal) of a hit by a segment of direction d"""
    front = dot(d, c.N) < 0.0
    return front, (c.N if front else (-c.N[0], -c.N[1], -c.N[2]))


def box_quads(mn, mx):
    """the six (Q, u, v) of an axis-aligned box in the header's order: front, right, back, left, top, bottom"""
    x0, y0, z0 = (float(v) for v in mn)
    x1, y1, z1 = (float(v) for v in mx)
    dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
    return [((x0, y0, z1), (dx, 0.0, 0.0), (0.0, dy, 0.0)), ((x1, y0, z1), (0.0, 0.0, -dz), (0.0, dy, 0.0)),
            ((x1, y0, z0), (-dx, 0.0, 0.0), (0.0, dy, 0.0)), ((x0, y0, z0), (0.0, 0.0, dz), (0.0, dy, 0.0)),
            ((x0, y1, z1), (dx, 0.0, 0.0), (0.0, 0.0, -dz)), ((x0, y0, z0), (dx, 0.0, 0.0), (0.0, 0.0, dz))]


class QuadMini(SM.SolidMini):
    def __init__(self, scene, atan2, center1=None, lens=None, quads=None):
        super().__init__(scene, atan2, center1, lens)
        self.n_spheres = len(self.obj)
        self.quads = list(quads) if quads is not None else []
        self.qc = [QuadConsts(tuple(q.q), tuple(q.u), tuple(q.v)) for q in self.quads]
        assert all(c.ok for c in self.qc)
        self.obj = self.obj + self.quads       # the material lookup: object n_spheres + k is quad k (same field names as RtSphere)

    def hit_world(self, o, d, node=0):
        hit = super().hit_world(o, d, node)    # every sphere first, in object order
        closest = self.last_t if hit is not None else M.F64_MAX
        best = None
        for k, c in enumerate(self.qc):        # then quad k before quad k + 1, strict
            r = quad_test(c, o, d, closest)
            if r is not None:
                closest, best = r[0], (k, r[1])
        if best is None:
            return hit
        k, P = best
        self.last_t = closest
        front, normal = quad_record(self.qc[k], d)
        return self.n_spheres + k, P, normal, front

    def centre_of(self, i):
        """the frame of a solid's pattern: the centre the hit test used, or a quad's Q"""
        return self.ct[i] if i < self.n_spheres else self.qc[i - self.n_spheres].Q

    def scatter(self, i, d, p, n, front, node):
        o = self.obj[i]
        if i >= self.n_spheres and o.kind in (SM.CHECKER, SM.NOISE):     # SolidMini.scatter with centre = Q
            sd = M.add(n, self.random_in_unit_sphere(node))
            if abs(sd[0]) < M.EPS and abs(sd[1]) < M.EPS and abs(sd[2]) < M.EPS:
                sd = n
            return M.sub(M.add(p, sd), p), SM.solid_colour(o, self.centre_of(i), p)
        return super().scatter(i, d, p, n, front, node)

    def aovs(self, n):
        """SolidMini.aovs with the quads: albedo by the material rule, the record's normal, 1 / t"""
        sc = self.sc
        out = np.zeros((sc.height, sc.width, 8), np.float32)
        for y in range(sc.height):
            for x in range(sc.width):
                acc = [0.0] * 8
                for s in range(n):
                    o, d = self.begin_sample(x, y, s)
                    hit = self.hit_world(o, d, 0)
                    if hit is None:
                        a = self.sky_colour(d)
                    else:
                        i, p, nrm, front = hit
                        ob = self.obj[i]
                        if ob.kind in (SM.CHECKER, SM.NOISE):
                            a = SM.solid_colour(ob, self.centre_of(i), p)
                        else:
                            a = (M.F(1.0),) * 3 if ob.kind in (M.GLASS, M.LIGHT) else tuple(M.F(v) for v in ob.albedo)
                        acc[3] += 1.0 / self.last_t
                        if nrm is not None:
                            acc[4] += nrm[0]; acc[5] += nrm[1]; acc[6] += nrm[2]
                        acc[7] += 1.0
                    for k in range(3):
                        acc[k] += float(a[k])
                out[y, x] = [np.float32(v / float(n)) for v in acc]
        return out

    def surface(self):
        """the surface record of DESIGN.md §19 for every pixel: (id u32, kind u32, t f64) of the pixel-centre pinhole ray's first hit —
        plain divisions, the camera origin, every sphere at shutter time 0.5, the medium draw at (this pixel, sample 0, node 0); a quad k
        is id n_spheres + k; a miss is (SURFACE_NONE, SURFACE_NONE, 0.0)"""
        sc = self.sc
        W, H = sc.width, sc.height
        org, ll, hor, ver = (tuple(v) for v in (sc.cam_origin, sc.cam_lower_left, sc.cam_horizontal, sc.cam_vertical))
        ids = np.full((H, W), SURFACE_NONE, np.uint32)
        kinds = np.full((H, W), SURFACE_NONE, np.uint32)
        ts = np.zeros((H, W), np.float64)
        self.set_tau(0.5)
        for y in range(H):
            for x in range(W):
                self.pixel, self.sample = y * W + x, 0
                u = (float(x) + 0.5) / float(W - 1)
                v = (float(H) - (float(y) + 0.5)) / float(H - 1)
                d = M.sub(M.add(M.add(ll, M.muls(hor, u)), M.muls(ver, v)), org)
                hit = self.hit_world(org, d, 0)
                if hit is not None:
                    ids[y, x], kinds[y, x], ts[y, x] = hit[0], self.obj[hit[0]].kind, self.last_t
        return ids, kinds, ts
