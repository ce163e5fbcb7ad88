"""The restatement of the solid textures, written from the contract's text (include/rt_abi.h, the issue that set it)
and not from csrc/common/rt_solid.h.

TEST INFRASTRUCTURE.  SolidMini is tests/medium_mini.py's MediumMini — shutter time, thin lens, media, the discarded count — with
scatter and the first-hit albedo overridden for spheres of kind RT_MAT_CHECKER and RT_MAT_NOISE.  The arithmetic is plain Python:
floats for f64 (CPython never fuses a * b + c), ints masked to 32 bits for the hash, math.floor for floor.
"""
import math
import struct

import numpy as np

import medium_mini as MM
import mini_oracle as M

CHECKER, NOISE = 6, 7
MODE_NOISE, MODE_TURBULENCE, MODE_MARBLE = 0, 1, 2
M32 = 0xFFFFFFFF
TWO52 = 4503599627370496.0
TWO31 = 2147483648.0
INV_2PI = 0.15915494309189535


def _finite(x):
    return x == x and abs(x) != math.inf


def checker_parity(p):
    """0: even, 1: odd"""
    f = []
    for x in p:
        if not _finite(x):
            return 0
        fl = math.floor(x)
        if not abs(float(fl)) < TWO52:
            return 0
        f.append(fl)
    return (f[0] + f[1] + f[2]) & 1


def corner_hash(ix, iy, iz, seed):
    h = ((ix * 0x9E3779B1) & M32) ^ ((iy * 0x85EBCA77) & M32) ^ ((iz * 0xC2B2AE3D) & M32) ^ seed
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def gradient(h, x, y, z):
    g = h & 15
    a = x if g < 8 else y
    b = y if g < 4 else (x if g in (12, 14) else z)
    return (-a if g & 1 else a) + (-b if g & 2 else b)


def noise(p, seed):
    for x in p:
        if not abs(x) < TWO31:         # (NaN compares false)
            return 0.0
    fl = [math.floor(x) for x in p]
    i = [f & M32 for f in fl]          # the int32 taken as u32
    t = [x - float(f) for x, f in zip(p, fl)]
    s = [v * v * (3.0 - 2.0 * v) for v in t]
    yv = []
    for dz in (0, 1):
        xv = []
        for dy in (0, 1):
            c = []
            for dx in (0, 1):
                h = corner_hash((i[0] + dx) & M32, (i[1] + dy) & M32, (i[2] + dz) & M32, seed)
                c.append(gradient(h, t[0] - float(dx), t[1] - float(dy), t[2] - float(dz)))
            xv.append(c[0] + s[0] * (c[1] - c[0]))
        yv.append(xv[0] + s[1] * (xv[1] - xv[0]))
    return yv[0] + s[2] * (yv[1] - yv[0])


def turbulence(p, octaves, seed):
    acc, w, r = 0.0, 1.0, tuple(p)
    for _ in range(octaves):
        acc += w * noise(r, seed)
        w *= 0.5
        r = (r[0] * 2.0, r[1] * 2.0, r[2] * 2.0)
    return abs(acc)


def factor(p, mode, octaves, seed):
    if mode == MODE_NOISE:
        f = 0.5 * (1.0 + noise(p, seed))
        return 0.0 if f < 0.0 else (1.0 if f > 1.0 else f)     # (N can pass 1 slightly: DESIGN.md §16 records the clamp)
    T = turbulence(p, octaves, seed)
    if mode == MODE_TURBULENCE:
        return T if T < 1.0 else 1.0
    x = INV_2PI * (p[2] + 10.0 * T)
    if not _finite(x):
        return 0.0
    s = x - float(math.floor(x))
    m = 1.0 - abs(2.0 * s - 1.0)
    return m * m * (3.0 - 2.0 * m)


def odd_colour(tex_w, tex_h):
    return tuple(M.F(struct.unpack("<f", struct.pack("<I", w & M32))[0]) for w in (tex_w, tex_w >> 32, tex_h))


def solid_colour(ob, centre, point):
    """the attenuation (three numpy.float32) of a hit at `point` on the Checker / Noise sphere `ob` whose centre the hit test used is `centre`"""
    q = M.sub(point, centre)
    sc = ob.h_offset
    p = (q[0] * sc, q[1] * sc, q[2] * sc)
    if ob.kind == CHECKER:
        return odd_colour(ob.tex_w, ob.tex_h) if checker_parity(p) else tuple(M.F(v) for v in ob.albedo)
    f = factor(p, ob.tex_id, ob.tex_w, ob.tex_h)
    return tuple(M.F(f * float(M.F(v))) for v in ob.albedo)


class SolidMini(MM.MediumMini):
    def scatter(self, i, d, p, n, front, node):
        o = self.obj[i]
        if o.kind in (CHECKER, NOISE):          # as Lambertian (mini_oracle.Mini.scatter), with the solid's colour
            sd = M.add(n, self.random_in_unit_sphere(node))
            if abs(sd[0]) < M.EPS and abs(sd[1]) < M.EPS and abs(sd[2]) < M.EPS:
                sd = n
            return M.sub(M.add(p, sd), p), solid_colour(o, self.ct[i], p)
        return super().scatter(i, d, p, n, front, node)

    def aovs(self, n):
        """MediumMini.aovs with the evaluated colour of a first hit on a solid"""
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
                        if ob.kind in (CHECKER, NOISE):
                            a = solid_colour(ob, self.ct[i], p)
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
