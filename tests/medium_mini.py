"""The restatement of participating media, written from the contract's text (include/rt_abi.h) alone.

TEST INFRASTRUCTURE.  MediumMini is tests/mini_oracle.py's Mini — plain Python floats for the f64 geometry, numpy.float32 for colour,
recursion as in the reference — with hit_world and scatter overridden for spheres of kind RT_MAT_MEDIUM, the shutter time of DESIGN.md
§14 and the thin lens of §13 for the camera ray, and rt_neg_log (csrc/common/rt_neg_log.h) restated in plain floats.  It counts the
segments of light loops started at a hit on a Light sphere separately (`discarded`: the reference computes and drops their sum,
raytracer.rs:124; the kernel never traces them), so that kernel.segments == segments - discarded can be asserted exactly.
"""
import math
import struct

import numpy as np

import mini_oracle as M

MEDIUM = 5
NODE_TIME = 0xFFFFFFFD
MEDIUM_SLOT = 0x80000000
T_MIN = 0.001

LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
L1, L2, L3, L4, L5, L6, L7 = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
                              1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)
SQRT2_MANT = 0x6A09E667F3BCD


def neg_log(x):
    """rt_neg_log restated: the steps of rt_neg_log.h's header, one IEEE operation each (CPython never fuses a * b + c)"""
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    k = 0
    e = bits >> 52
    if e == 0 or e >= 0x7FF:
        if (bits << 1) & 0xFFFFFFFFFFFFFFFF == 0:
            return math.inf
        if bits >> 63 or x != x:
            return math.nan
        if e == 0x7FF:
            return -math.inf
        x = x * 18014398509481984.0
        k = -54
        bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    k += (bits >> 52) - 1023
    mant = bits & 0x000FFFFFFFFFFFFF
    if mant >= SQRT2_MANT:
        mb = (1022 << 52) | mant
        k += 1
    else:
        mb = (1023 << 52) | mant
    m = struct.unpack("<d", struct.pack("<Q", mb))[0]
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (L2 + w * (L4 + w * L6))
    t2 = z * (L1 + w * (L3 + w * (L5 + w * L7)))
    R = t2 + t1
    hfsq = (0.5 * f) * f
    dk = float(k)
    return ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f) - dk * LN2_HI


def medium_candidate(o, d, c, r, density, u):
    """the contract's candidate t of one medium sphere (centre c, radius r) for the ray (o, d) and the draw u, or None"""
    a = M.len2(d)
    oc = M.sub(o, c)
    half_b = M.dot(oc, d)
    cc = M.len2(oc) - r * r
    disc = (half_b * half_b) - (a * cc)
    if not disc >= 0.0:
        return None
    sq = math.sqrt(disc)
    t1, t2 = ((-half_b) - sq) / a, ((-half_b) + sq) / a
    t_in = t1 if t1 > T_MIN else T_MIN
    if not t_in < t2:
        return None
    ln = math.sqrt(a)
    inside = (t2 - t_in) * ln
    dist = neg_log(1.0 - u) / density
    if not dist <= inside:
        return None
    return t_in + dist / ln


def dv_of(c0, c1):
    return tuple(-0.0 if (b == a or (a != a and b != b)) else b - a for a, b in zip(c0, c1))


class MediumMini(M.Mini):
    def __init__(self, scene, atan2, center1=None, lens=None):
        super().__init__(scene, atan2)
        self.c0 = [tuple(o.center) for o in self.obj]
        self.dv = [dv_of(c0, tuple(c1)) for c0, c1 in zip(self.c0, center1)] if center1 is not None else None
        self.lens = lens
        self.ct = list(self.c0)
        self.discarded = 0
        self._in_discard = False

    def set_tau(self, tau):
        if self.dv is not None:
            self.ct = [(c[0] + d[0] * tau, c[1] + d[1] * tau, c[2] + d[2] * tau) for c, d in zip(self.c0, self.dv)]

    def hit_world(self, o, d, node=0):
        closest, best = M.F64_MAX, None
        a = M.len2(d)
        for i, c in enumerate(self.ct):
            ob = self.obj[i]
            r = ob.radius
            if ob.kind == MEDIUM:
                w = self.words(node, MEDIUM_SLOT | i)
                t = medium_candidate(o, d, c, r, ob.fuzz_or_ior, M.u01_53(w[0], w[1]))
                if t is not None and t > T_MIN and t < closest:
                    closest, best = t, i
                continue
            oc = M.sub(o, c)
            half_b = M.dot(oc, d)
            cc = M.len2(oc) - r * r
            disc = (half_b * half_b) - (a * cc)
            if disc >= 0.0:
                sq = math.sqrt(disc)
                for root in (((-half_b) - sq) / a, ((-half_b) + sq) / a):
                    if root < closest and root > T_MIN:
                        closest, best = root, i
                        break
        if best is None:
            return None
        self.last_t = closest
        p = M.add(o, M.muls(d, closest))
        if self.obj[best].kind == MEDIUM:
            return best, p, None, True
        c, r = self.ct[best], self.obj[best].radius
        normal = M.divs(M.sub(p, c), r)
        front = M.dot(d, normal) < 0.0
        return best, p, (normal if front else M.neg(normal)), front

    def scatter(self, i, d, p, n, front, node):
        o = self.obj[i]
        if o.kind == MEDIUM:
            sd = self.random_in_unit_sphere(node)
            if abs(sd[0]) < M.EPS and abs(sd[1]) < M.EPS and abs(sd[2]) < M.EPS:
                sd = d
            return sd, tuple(M.F(x) for x in o.albedo)
        return super().scatter(i, d, p, n, front, node)

    def ray_color(self, o, d, max_depth, depth, node, nest):     # Mini.ray_color with the node handed to hit_world and the discarded count
        F = M.F
        if depth <= 0:
            return F(0.0), F(0.0), F(0.0)
        self.segments += 1
        if self._in_discard:
            self.discarded += 1
        hit = self.hit_world(o, d, node)
        if hit is None:
            return self.sky_colour(d)
        i, p, n, front = hit
        sc = self.scatter(i, d, p, n, front, node)
        if sc is None:
            return F(0.0), F(0.0), F(0.0)
        sdir, alb = sc
        light = [F(0.0), F(0.0), F(0.0)]
        nl = len(self.lights)
        glass = self.obj[i].kind == M.GLASS
        prob = 0.05 if glass else 0.1
        if nl > 0:
            w0 = self.words(node, 0)
            draw = M.u01_53(w0[2], w0[3]) if glass else M.u01_53(w0[2], self.words(node, 1)[3])
            if draw > (1.0 - float(nl) * prob) and depth > ((max_depth - 2) % 2 ** 64) and nest < M.MAX_LIGHT_NEST:
                mark = sdir is None and not self._in_discard   # a Light hit: the loop's sum is dropped (raytracer.rs:124)
                if mark:
                    self._in_discard = True
                for j, li in enumerate(self.lights):
                    tc = self.ray_color(p, M.sub(self.ct[li], p), 2, 1, M.child_node(node, j), nest + 1)
                    for k in range(3):
                        light[k] = light[k] + alb[k] * tc[k]
                light = [x / F(nl) for x in light]
                if mark:
                    self._in_discard = False
        if sdir is None:
            return alb
        tc = self.ray_color(p, sdir, max_depth, depth - 1, node + 1, nest)
        return tuple(M.clamp(light[k] + alb[k] * tc[k]) for k in range(3))

    def camera_ray(self, x, y):
        sc = self.sc
        W, H = sc.width, sc.height
        org, ll, hor, ver = (tuple(v) for v in (sc.cam_origin, sc.cam_lower_left, sc.cam_horizontal, sc.cam_vertical))
        w = self.words(M.NODE_CAMERA, 0)
        u = (float(x) + M.u01_53(w[0], w[1])) / (float(W) - 1.0)
        v = (float(H) - (float(y) + M.u01_53(w[2], w[3]))) / (float(H) - 1.0)
        d = M.sub(M.add(M.add(ll, M.muls(hor, u)), M.muls(ver, v)), org)
        if self.lens is None:
            return org, d
        lu, lv, r = self.lens
        a = 0
        while True:                               # the lens point: NODE_CAMERA slots 1, 2, ...
            ww = self.words(M.NODE_CAMERA, 1 + a)
            pt = None
            for p, q in ((ww[0], ww[1]), (ww[2], ww[3])):
                px, py = M.range_m1_1(p), M.range_m1_1(q)
                if px * px + py * py < 1.0:
                    pt = (px, py)
                    break
            if pt is not None:
                break
            a += 1
        off = M.add(M.muls(tuple(lu), r * pt[0]), M.muls(tuple(lv), r * pt[1]))
        return M.add(org, off), M.sub(d, off)

    def begin_sample(self, x, y, s):
        self.pixel, self.sample = y * self.sc.width + x, s
        if self.dv is not None:
            self.set_tau(float(self.words(NODE_TIME, 0)[0] >> 8) * 2.0 ** -24)
        return self.camera_ray(x, y)

    def render(self):
        sc = self.sc
        W, H, spp = sc.width, sc.height, sc.samples_per_pixel
        lin, rgb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.uint8)
        for y in range(H):
            for x in range(W):
                acc = [M.F(0.0), M.F(0.0), M.F(0.0)]
                for s in range(spp):
                    o, d = self.begin_sample(x, y, s)
                    c = self.ray_color(o, d, sc.max_depth, sc.max_depth, 0, 0)
                    acc = [acc[k] + c[k] for k in range(3)]
                scale = M.F(1.0) / M.F(spp)
                for k in range(3):
                    lin[y, x, k] = scale * acc[k]
                    g = np.sqrt(scale * acc[k]) * M.F(255.0)
                    rgb[y, x, k] = 255 if g != g else int(np.rint(min(max(g, M.F(0.0)), M.F(255.0))))
        return rgb, lin, self.segments

    def aovs(self, n):
        """the first-hit record of DESIGN.md §12 (albedo, 1 / t, normal, coverage: means over samples [0, n) in f64, rounded once) for
        scenes of Lambertian, Metal, Glass, Light and Medium spheres"""
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
                        a = (M.F(1.0),) * 3 if ob.kind in (M.GLASS, M.LIGHT) else tuple(M.F(v) for v in ob.albedo)
                        acc[3] += 1.0 / self.last_t
                        if nrm is not None:
                            acc[4] += nrm[0]; acc[5] += nrm[1]; acc[6] += nrm[2]
                        acc[7] += 1.0
                    for k in range(3):
                        acc[k] += float(a[k])
                out[y, x] = [np.float32(v / float(n)) for v in acc]
        return out
