"""The restatement of images on flat primitives, written from the contract's text (the issue that set it: section 1, "The
contract") and not from the header or the kernel.

TEST INFRASTRUCTURE.  Per entry an image is (s, t) at Q, at Q + u and at Q + v, a texture of W x H texels (the DECODED size), and a wrap
mode per axis.  Per accepted hit at P on an entry whose origin at the sample's shutter time is O:
    p = P - O      alpha = dot(w, cross(p, v))      beta = dot(w, cross(u, p))      gamma = (1 - alpha) - beta
    s = (s0 gamma + s1 alpha) + s2 beta             t likewise
    REPEAT: x' = x - floor(x), and x' = 0 unless x' < 1        CLAMP: x' = min(max(x, 0), 1), a NaN: 0
    col = min(floor(s' W), W - 1)      row = min(floor((1 - t') H), H - 1)      index = texel_off + row W + col
    colour = bytes / 255 in f32
An entry with an image scatters as its own material (Lambertian or Metal) does; its attenuation is the texel.  An entry that emits, emits.
Plain Python floats: CPython never fuses a * b + c.
"""
import math

import numpy as np

import flat_light_mini as LM
import mini_oracle as M
import quad_mini as QM
import solid_mini as SM

NONE = 0xFFFFFFFF
REPEAT, CLAMP = 0, 1
ABSENT, PRESENT, BAD_UV, BAD_TEX_ID, BAD_TEX_SIZE, BAD_TEX_FAR, BAD_WRAP, BAD_RESERVED, BAD_MATERIAL = range(9)


def _finite(x):
    return x == x and abs(x) != math.inf


def _floor(x):
    """floor of a float as a float; NaN and the infinities stay what they are"""
    return float(math.floor(x)) if _finite(x) else x


def wrap(x, mode):
    if mode == CLAMP:
        if x != x:
            return 0.0
        x = x if x > 0.0 else 0.0
        return x if x < 1.0 else 1.0
    f = x - _floor(x)                      # (inf - inf: NaN)
    return f if f < 1.0 else 0.0


def tex_table(textures):
    """[(texel_off, W, H, ok)] of a scene's textures [(width, height, nbytes)]: back to back, the first 2^31 texels"""
    out, before = [], 0
    for (w, h, nbytes) in textures:
        if w == 0 or h == 0 or nbytes != 3 * w * h:
            out.append((0, w, h, 2))
        elif before + nbytes // 3 >= 2 ** 31:
            out.append((0, w, h, 3))
        else:
            out.append((before, w, h, 1))
        before = 2 ** 31 if (out[-1][3] == 3 or before + nbytes // 3 >= 2 ** 31) else before + nbytes // 3
    return out


def prepare(uv, tex_id, wrap_s, wrap_t, reserved, table, kind):
    """(code, record) of one entry; record = (texel_off, W, H, wrap_s | wrap_t << 1, uv) or None"""
    if tex_id == NONE:
        return ABSENT, (0, 0, 0, 0, (0.0,) * 6)
    if not all(_finite(float(x)) for x in uv):
        return BAD_UV, None
    if tex_id >= len(table):
        return BAD_TEX_ID, None
    off, w, h, ok = table[tex_id]
    if ok == 3:
        return BAD_TEX_FAR, None
    if ok != 1:
        return BAD_TEX_SIZE, None
    if wrap_s > 1 or wrap_t > 1:
        return BAD_WRAP, None
    if reserved != 0:
        return BAD_RESERVED, None
    if kind not in (M.LAMBERTIAN, M.METAL):
        return BAD_MATERIAL, None
    return PRESENT, (off, w, h, wrap_s | (wrap_t << 1), tuple(float(x) for x in uv))


def texel(rec, O, u, v, w, P):
    """(col, row, index) of the hit at P"""
    off, W, H, wr, uv = rec
    p = (P[0] - O[0], P[1] - O[1], P[2] - O[2])
    alpha = QM.dot(w, QM.cross(p, v))
    beta = QM.dot(w, QM.cross(u, p))
    gamma = (1.0 - alpha) - beta
    s = (uv[0] * gamma + uv[2] * alpha) + uv[4] * beta
    t = (uv[1] * gamma + uv[3] * alpha) + uv[5] * beta
    sw, tw = wrap(s, wr & 1), wrap(t, (wr >> 1) & 1)
    col = min(int(math.floor(sw * float(W))), W - 1)
    row = min(int(math.floor((1.0 - tw) * float(H))), H - 1)
    return col, row, off + row * W + col


def colour(px, index_in_texture):
    """the three f32 of texel `index_in_texture` of the RGB8 array px"""
    return tuple(M.F(px[3 * index_in_texture + k]) / M.F(255.0) for k in range(3))


class FlatImageMini(LM.FlatLightMini):
    """FlatLightMini whose entries may show an image (images: a sequence of abi.RtFlatImage, or None)"""

    def __init__(self, scene, atan2, center1=None, lens=None, quads=None, normals=None, move=None, emit=None, images=None):
        super().__init__(scene, atan2, center1, lens, quads, normals, move, emit)
        self.image = {}
        self.image_hits = {}                # entry -> the lookups it served (a frame that never sees its image shows nothing)
        if images is not None:
            assert len(images) == len(self.quads)
            table = tex_table([(scene.textures[i].width, scene.textures[i].height, scene.textures[i].nbytes) for i in range(scene.n_textures)])
            for k, im in enumerate(images):
                code, rec = prepare(list(im.uv), im.tex_id, im.wrap_s, im.wrap_t, im.reserved, table, self.quads[k].kind)
                assert code in (ABSENT, PRESENT), (k, code)
                if code == PRESENT:
                    self.image[k] = (rec, im.tex_id, table[im.tex_id][0])

    def image_colour(self, k, p):
        rec, tex_id, off = self.image[k]
        c = self.qc[k]                      # (at the sample's shutter time in a scene whose entries move)
        _, _, index = texel(rec, c.Q, c.u, c.v, c.w, p)
        self.image_hits[k] = self.image_hits.get(k, 0) + 1
        return colour(self.tex[tex_id], index - off)

    def scatter(self, i, d, p, n, front, node):
        sc = super().scatter(i, d, p, n, front, node)
        k = i - self.n_spheres
        if sc is None or sc[0] is None or k < 0 or k not in self.image or k in self.emit:
            return sc
        return sc[0], self.image_colour(k, p)

    def aovs(self, n):
        """FlatLightMini.aovs; a first hit on an entry with an image (that does not emit) reports its texel"""
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
                        k = i - self.n_spheres
                        if k in self.emit:
                            a = self.emit[k]
                        elif k in self.image:
                            a = self.image_colour(k, p)
                        elif ob.kind in (SM.CHECKER, SM.NOISE):
                            a = SM.solid_colour(ob, self.centre_of(i), p)
                        else:
                            a = (M.F(1.0),) * 3 if ob.kind in (M.GLASS, M.LIGHT) else tuple(M.F(v) for v in ob.albedo)
                        acc[3] += 1.0 / self.last_t
                        if nrm is not None:
                            acc[4] += nrm[0]; acc[5] += nrm[1]; acc[6] += nrm[2]
                        acc[7] += 1.0
                    for c in range(3):
                        acc[c] += float(a[c])
                out[y, x] = [np.float32(v / float(n)) for v in acc]
        return out
