"""The worlds of the parity frames of images on flat primitives and the restatement's frames of them, computed once per
session and left unchanged: the CPU and the GPU tests share them.  TEST INFRASTRUCTURE.

The textures are synthetic RGB8 arrays of 8 x 4, 5 x 3 and 1 x 1 texels handed over through RtTexture (attach); an object of a case's
scene names its image under the private key "_img", taken out before the file is loaded: {"tex", "uv" (six floats; None: the default; a
function of a vertex for a mesh), "wrap" (ws, wt)}."""
import copy
import ctypes as C

import numpy as np

import flat_image_mini as IM
import flat_light_frames as LF
import smooth_worlds as SW
from test_medium_gpu import _cfg, _lam, _load, _obj
from test_quad_gpu import GLASS, LENS_KEYS, _box, _floor_objs, _metal, _quad, _room_objs

W, H, SPP, DEPTH = 48, 32, 4, 8
PARITY_CASES = ["poster", "metal_fuzz", "smooth_mesh", "lens_moving_sphere", "moving_quad", "under_lamp", "image_and_emit"]
TEX_SIZES = [(8, 4), (5, 3), (1, 1)]
WHITE = _lam(0.73, 0.73, 0.73)
_CACHE = {}


def texture_arrays():
    """the three textures: every texel its own colour, no two alike within a texture"""
    rng = np.random.default_rng(2909)
    out = []
    for w, h in TEX_SIZES:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[..., 0] = (np.arange(w * h).reshape(h, w) * 7 + 3) % 256      # (red tells the texel)
        out.append(np.ascontiguousarray(a))
    return out


def attach(abi, sc, arrays=None):
    """point the host scene's RtScene at the synthetic textures; returns what must stay alive as long as the scene is used"""
    arrays = texture_arrays() if arrays is None else arrays
    tex = (abi.RtTexture * len(arrays))()
    for i, a in enumerate(arrays):
        tex[i].rgb8 = a.ctypes.data_as(C.POINTER(C.c_uint8))
        tex[i].nbytes = a.size
        tex[i].height, tex[i].width = a.shape[0], a.shape[1]
    sc.c.textures = tex
    sc.c.n_textures = len(arrays)
    return tex, arrays


def img(o, tex, uv=None, wrap=(0, 0)):
    o = copy.deepcopy(o)
    o["_img"] = {"tex": tex, "uv": uv, "wrap": wrap}
    return o


def _entries(o):
    """the flat entries an object of the file becomes (0: a sphere)"""
    if "box" in o:
        return 6
    if "mesh" in o:
        return len(o["mesh"]["faces"])
    return 1 if ("q" in o or "triangle" in o) else 0


def split(abi, cfg):
    """(the file's cfg without the private key, the RtFlatImage of every entry)"""
    cfg = copy.deepcopy(cfg)
    images = []
    for o in cfg["objects"]:
        spec = o.pop("_img", None) if isinstance(o, dict) else None
        for f in range(_entries(o) if isinstance(o, dict) else 0):
            if spec is None:
                images.append(abi.flat_image())
                continue
            uv = spec["uv"]
            if callable(uv):
                vs = o["mesh"]["vertices"]
                uv = [c for ix in o["mesh"]["faces"][f] for c in uv(vs[ix])]
            images.append(abi.flat_image(spec["tex"], uv or (0.0, 0.0, 1.0, 0.0, 0.0, 1.0), *spec["wrap"]))
    return cfg, (abi.RtFlatImage * len(images))(*images)


def _room_cfg(objs, lens=None):
    return _cfg(objs, sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0), lens=lens)


def parity_cfg(case):
    if case == "poster":               # the lit room, a Lambertian poster on its back wall and a tiled floor
        objs = _room_objs()
        objs[2] = img(objs[2], 0)
        objs[0] = img(objs[0], 1, (0.0, 0.0, 3.0, 0.0, 0.0, 3.0))
        return _room_cfg(objs)
    if case == "metal_fuzz":           # the fuzzy Metal quad behind the spheres: negative and tiling uv, repeat in s, clamp in t
        objs = _floor_objs()
        objs[3] = img(objs[3], 1, (-1.0, -0.5, 2.0, -0.5, -1.0, 1.5), (0, 1))
        return _cfg(objs)
    if case == "smooth_mesh":          # a smooth Metal icosphere with per-vertex uv, and a one-texel box
        mesh = img(SW.ico_mesh(0, (1.0, 0.3, -0.6), 0.7, _metal((0.9, 0.9, 0.95), 0.05)), 0, lambda p: (0.9 * p[0] + 0.3 * p[2], 1.1 * p[1] + 0.2))
        objs = _room_objs()
        objs[6] = img(objs[6], 2)
        return _room_cfg(objs + [mesh])
    if case == "lens_moving_sphere":   # a thin lens and a moving sphere over a tiled floor
        objs = _floor_objs(moving=True)
        objs[0] = img(objs[0], 0, (0.0, 0.0, 5.0, 0.0, 0.0, 5.0))
        return _cfg(objs, lens=LENS_KEYS)
    if case == "moving_quad":          # an image on a quad that moves while the shutter is open: the frame of its (s, t) moves with it
        objs = _room_objs()
        sign = img(_quad((-0.9, 0.2, 0.4), (1.4, 0, 0.2), (0, 1.0, 0), WHITE), 0, None, (1, 1))
        sign["move"] = [0.8, 0.3, 0.0]
        return _room_cfg(objs + [sign])
    if case == "under_lamp":           # the poster lit by a ceiling panel instead of the sphere
        objs = LF.room(LF.panel())
        objs[2] = img(objs[2], 0)
        return _room_cfg(objs)
    if case == "image_and_emit":       # an entry with both: it emits, the image is not looked at
        objs = LF.room(img(LF.panel(), 1))
        objs[2] = img(objs[2], 0)
        return _room_cfg(objs)
    raise KeyError(case)


def world(host, abi, case, cfg=None):
    """{sc, c1, lens, quads, normals, move, emit, images, keep} of one parity case"""
    cfg, images = split(abi, cfg or parity_cfg(case))
    sc, c1, lens = _load(host, cfg, W, H, SPP, DEPTH, seed=173)
    keep = attach(abi, sc)
    quads = sc.quads()
    assert len(quads) == len(images)
    return {"sc": sc, "c1": c1, "lens": lens, "quads": quads, "normals": sc.flat_normals(), "move": sc.flat_motion(), "emit": sc.flat_emit(),
            "images": images, "keep": keep}


def mini(oracle, abi, w, images="own"):
    L = oracle.lib(abi)
    return IM.FlatImageMini(w["sc"].c, lambda y, x: L.rt_oracle_atan2(y, x), w["c1"], w["lens"], w["quads"], w["normals"], w["move"], w["emit"],
                            w["images"] if images == "own" else images)


def mini_frame(oracle, abi, host, case):
    if case not in _CACHE:
        w = world(host, abi, case)
        m = mini(oracle, abi, w)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _CACHE[case] = {"rgb": rgb, "lin": lin, "segments": segs, "discarded": m.discarded, "hits": dict(m.image_hits)}
    return _CACHE[case]


# ------------------------------------------------------------------ the constant-image identity: a check that needs no restatement
CONST_COLOUR = (200, 30, 117)


def constant_pair(host, abi, div255):
    """(world with a one-colour image on the room's back wall, the same world without images whose wall has albedo = div255(colour))"""
    objs = _room_objs()
    with_image = copy.deepcopy(objs)
    with_image[2] = img(with_image[2], 0, (-2.0, 0.3, 4.0, 0.1, 0.5, 7.0))
    cfg, images = split(abi, _room_cfg(with_image))
    sc, c1, lens = _load(host, cfg, W, H, SPP, DEPTH, seed=59)
    flat = np.zeros((3, 7, 3), np.uint8); flat[...] = CONST_COLOUR
    keep = attach(abi, sc, [flat])
    a = {"sc": sc, "c1": c1, "lens": lens, "quads": sc.quads(), "normals": None, "move": None, "emit": None, "images": images, "keep": keep}
    sc2, c12, lens2 = _load(host, cfg, W, H, SPP, DEPTH, seed=59)
    quads2 = sc2.quads()
    for k in range(3):
        quads2[2].albedo[k] = div255(CONST_COLOUR[k])
    b = {"sc": sc2, "c1": c12, "lens": lens2, "quads": quads2, "normals": None, "move": None, "emit": None, "images": None, "keep": None}
    return a, b
