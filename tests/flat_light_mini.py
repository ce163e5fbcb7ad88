"""The restatement of flat primitives that emit and are sampled, written from the contract's text (the header comment of
csrc/common/rt_flat_light.h, include/rt_abi.h at rt_hip_scene_set_flat_lights, the issue that set it) and not from the kernel.

TEST INFRASTRUCTURE.  `emit` is [n_quads][3] f32; an entry of three zeros does not emit, any other is an emitter: it scatters as Light
does (no scattered ray), its colour is `emit`, from both faces; its own material is ignored.  The light list is the Light spheres in
object order, then the emitters in entry order; n_lights is the total.  Light j that is emitter entry k, shot from a hit at P whose
activation has RNG node `node`:
    c = child_node(node, j)      w = words(c, 0xFFFFFFFF)      a = u01_53(w0, w1)      b = u01_53(w2, w3)
    triangle only: if a + b > 1.0: a = 1.0 - a; b = 1.0 - b
    T_k = (Q_k + u_k a) + v_k b      d = T - P
A Light sphere is aimed at its centre, no draw.  Plain Python floats: CPython never fuses a * b + c.
"""
import types

import numpy as np

import flat_motion_mini as FM
import mini_oracle as M
import solid_mini as SM

AIM_SLOT = 0xFFFFFFFF
MAX_FLAT_LIGHTS = 32


def component_ok(c):
    c = float(c)
    return c >= 0.0 and c <= 1.0           # (a NaN fails both)


def emits(e):
    return not (float(e[0]) == 0.0 and float(e[1]) == 0.0 and float(e[2]) == 0.0)


def emit_check(emit):
    """(the lowest entry with a bad component or len(emit), the emitters' entry indices)"""
    for k, e in enumerate(emit):
        if not all(component_ok(c) for c in e):
            return k, None
    return len(emit), [k for k, e in enumerate(emit) if emits(e)]


def u01(lo, hi):
    return M.u01_53(lo, hi)


def aim(Q, u, v, triangle, w):
    """the point of the entry {Q, u, v} the four words aim at"""
    a, b = u01(w[0], w[1]), u01(w[2], w[3])
    if triangle and a + b > 1.0:
        a = 1.0 - a
        b = 1.0 - b
    return tuple((Q[k] + u[k] * a) + v[k] * b for k in range(3))


class FlatLightMini(FM.FlatMotionMini):
    """FlatMotionMini whose entries may emit (emit: [n_quads][3] f32 as given, or None)"""

    def __init__(self, scene, atan2, center1=None, lens=None, quads=None, normals=None, move=None, emit=None):
        super().__init__(scene, atan2, center1, lens, quads, normals, move)
        self.emit = {}
        if emit is not None:
            assert len(emit) == len(self.quads)
            bad, emitters = emit_check(emit)
            assert bad == len(emit) and len(emitters) <= MAX_FLAT_LIGHTS
            if move is not None:
                assert all(not any(float(x) != 0.0 for x in move[k]) for k in emitters), "an emitter cannot move"
            for k in emitters:
                col = tuple(M.F(c) for c in emit[k])
                self.emit[k] = col
                # the material lookup: while it emits the entry is a Light of colour `emit`, whatever its own material
                self.obj[self.n_spheres + k] = types.SimpleNamespace(kind=M.LIGHT, albedo=col, fuzz_or_ior=0.0, h_offset=0.0, tex_w=0, tex_h=0, tex_id=0)
            self.lights = self.lights + [self.n_spheres + k for k in emitters]     # Light spheres, then the emitters in entry order

    def scatter(self, i, d, p, n, front, node):
        k = i - self.n_spheres
        if k >= 0 and k in self.emit:
            return None, self.emit[k]
        return super().scatter(i, d, p, n, front, node)

    def light_direction(self, li, j, p, node):
        """the direction of the light ray of light j (object li) shot from p by the activation of RNG node `node`"""
        if li < self.n_spheres:
            return M.sub(self.ct[li], p)
        k = li - self.n_spheres
        c = self.qc[k]
        T = aim(c.Q, c.u, c.v, self.lim[k] == 1.0, self.words(M.child_node(node, j), AIM_SLOT))
        return M.sub(T, p)

    def ray_color(self, o, d, max_depth, depth, node, nest):     # MediumMini.ray_color with the aim above
        F = M.F
        if depth <= 0:
            return F(0.0), F(0.0), F(0.0)
        self.segments += 1
        hit = self.hit_world(o, d, node)
        if hit is None:
            return self.sky_colour(d)
        i, p, n, front = hit
        sc = self.scatter(i, d, p, n, front, node)
        if sc is None:
            return F(0.0), F(0.0), F(0.0)
        sdir, alb = sc
        if sdir is None:
            # A hit on a Light.  The reference runs the light loop here too and drops its sum (raytracer.rs:124); MediumMini traces that
            # loop and counts its segments as `discarded`.  Nothing depends on it — the draws are counter-addressed — and with six lights
            # (threshold 0.4) eight levels of dropped loops are 3.6^8 segments per hit: this restatement leaves them out of both counts
            # (discarded stays 0), so that segments - discarded is what it was.
            return alb
        light = [F(0.0), F(0.0), F(0.0)]
        nl = len(self.lights)
        glass = self.obj[i].kind == M.GLASS
        prob = 0.05 if glass else 0.1
        if nl > 0:
            w0 = self.words(node, 0)
            draw = M.u01_53(w0[2], w0[3]) if glass else M.u01_53(w0[2], self.words(node, 1)[3])
            if draw > (1.0 - float(nl) * prob) and depth > ((max_depth - 2) % 2 ** 64) and nest < M.MAX_LIGHT_NEST:
                for j, li in enumerate(self.lights):
                    tc = self.ray_color(p, self.light_direction(li, j, p, node), 2, 1, M.child_node(node, j), nest + 1)
                    for k in range(3):
                        light[k] = light[k] + alb[k] * tc[k]
                light = [x / F(nl) for x in light]
        tc = self.ray_color(p, sdir, max_depth, depth - 1, node + 1, nest)
        return tuple(M.clamp(light[k] + alb[k] * tc[k]) for k in range(3))

    def aovs(self, n):
        """QuadMini.aovs; a first hit on an emitter reports albedo `emit`"""
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
                        if i - self.n_spheres in self.emit:
                            a = self.emit[i - self.n_spheres]
                        elif ob.kind in (SM.CHECKER, SM.NOISE):
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
