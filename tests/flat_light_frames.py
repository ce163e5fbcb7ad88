"""The worlds of the parity frames of flat primitives that emit and the restatement's frames of them, computed once per
session and left unchanged: the CPU and the GPU tests share them.  TEST INFRASTRUCTURE."""
import copy

import numpy as np

import flat_light_mini as LM
import smooth_worlds as SW
from test_medium_gpu import _cfg, _lam, _load, _med, _obj
from test_quad_gpu import GLASS, LENS_KEYS, _box, _chk, _metal, _quad, _room_objs

W, H, SPP, DEPTH = 48, 32, 4, 8
PARITY_CASES = ["room_panel", "tri_lamp", "panel_sphere", "box_lamp", "lens", "moving_sphere", "medium", "checker", "glass_pane", "smooth_mesh"]
CPU_CASES = list(PARITY_CASES)                              # the lens frame through tests/flatlight/flat_light_sim.cpp's own loop
WARM = [1.0, 0.9, 0.75]
WHITE = _lam(0.73, 0.73, 0.73)
_CACHE = {}


def emitting(o, e):
    o = copy.deepcopy(o)
    o["emit"] = [float(x) for x in e]
    return o


def panel(e=WARM, half=0.6, y=2.98):
    """the ceiling panel of the room of tests/test_quad_gpu.py: a square just under the ceiling quad"""
    return emitting(_quad((-half, y, -half), (2 * half, 0, 0), (0, 0, 2 * half), WHITE), e)


def room(lamp, extra=(), keep_sphere=False):
    """the room with its Light sphere replaced by `lamp` (keep_sphere: beside it)"""
    objs = _room_objs()
    assert "Light" in objs[3]["material"]
    if keep_sphere:
        objs.insert(4, lamp)
    else:
        objs[3] = lamp
    return objs + list(extra)


def _room_cfg(objs, lens=None):
    return _cfg(objs, sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0), lens=lens)


def parity_cfg(case):
    """48 x 32 scenes written with "emit" in the file, so that the loader's table is what the scene is given"""
    if case == "room_panel":            # the room with a ceiling panel
        return _room_cfg(room(panel()))
    if case == "tri_lamp":              # a triangle lamp: the fold
        return _room_cfg(room(emitting({"triangle": [[-0.9, 2.98, -0.8], [1.0, 2.98, -0.5], [0.1, 2.98, 0.9]], "material": WHITE}, (0.9, 1.0, 0.8))))
    if case == "panel_sphere":          # a panel plus the Light sphere: the sphere is light 0, the panel light 1, / 2
        return _room_cfg(room(emitting(_quad((-2, 0.5, -0.5), (0, 0, 1.0), (0, 1.0, 0), WHITE), (0.3, 0.5, 1.0)), keep_sphere=True))
    if case == "box_lamp":              # a box lamp: six lights, threshold 0.4
        return _room_cfg(room(emitting(_box((-0.4, 2.3, -0.4), (0.4, 2.7, 0.4), WHITE), (1.0, 1.0, 0.9))))
    if case == "lens":
        return _room_cfg(room(panel()), lens=LENS_KEYS)
    if case == "moving_sphere":         # MOTION with a still emitter
        objs = room(panel())
        objs[8] = _obj((0.2, -0.7, 1.2), 0.3, _lam(0.3, 0.3, 0.8), (0.7, -0.3, 1.0))
        return _room_cfg(objs)
    if case == "medium":                # a Medium sphere in the beam
        return _room_cfg(room(panel(), extra=[_obj((0.0, 1.4, 0.0), 0.9, _med((0.9, 0.9, 0.9), 1.5))]))
    if case == "checker":               # a Checker floor
        objs = room(panel())
        objs[0] = _quad((-2, -1, -2), (4, 0, 0), (0, 0, 4), _chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 0.4))
        return _room_cfg(objs)
    if case == "glass_pane":            # a Glass pane between lamp and floor: the 0.05 threshold
        return _room_cfg(room(panel(), extra=[_quad((-1.2, 1.6, -1.2), (2.4, 0, 0), (0, 0, 2.4), GLASS)]))
    if case == "smooth_mesh":           # smooth normals on a lit mesh
        return _room_cfg(room(panel(), extra=[SW.ico_mesh(0, (1.0, 0.3, -0.6), 0.7, _metal((0.9, 0.9, 0.95), 0.05))]))
    raise KeyError(case)


def world(host, case, cfg=None):
    """(host scene, center1, lens, quads, normals [n, 9] or None, emit [n, 3] f32) of one parity case"""
    sc, c1, lens = _load(host, cfg or parity_cfg(case), W, H, SPP, DEPTH, seed=151)
    emit = sc.flat_emit()
    assert emit is not None and (emit != 0).any() and emit.dtype == np.float32
    return sc, c1, lens, sc.quads(), sc.flat_normals(), emit


def mini(oracle, abi, sc, c1, lens, quads, normals, emit):
    L = oracle.lib(abi)
    return LM.FlatLightMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), c1, lens, quads, normals, None, emit)


def mini_frame(oracle, abi, host, case):
    if case not in _CACHE:
        sc, c1, lens, quads, normals, emit = world(host, case)
        m = mini(oracle, abi, sc, c1, lens, quads, normals, emit)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _CACHE[case] = {"rgb": rgb, "lin": lin, "segments": segs, "discarded": m.discarded, "n_lights": len(m.lights)}
    return _CACHE[case]


# ------------------------------------------------------------------ the colour check (tests/test_flat_light_gpu.py::test_colour)
def colour_cfg(emitting_panel):
    """the room with a pure red panel; or (False) the same room whose panel does not emit, with a Light sphere of radius 1e-3 far behind
    the back wall inside a closed box of albedo 0: a light ray towards it from inside the room ends on the back wall, one from the back
    wall itself (t_min lets it leave) on the box, whose albedo multiplies whatever its own light loop returns by 0"""
    objs = room(panel((1.0, 0.0, 0.0)))
    if not emitting_panel:
        objs[3].pop("emit")
        objs.append(_obj((0.0, 1.0, -50.0), 1e-3, {"Light": {}}))
        objs.append(_box((-1.0, 0.0, -51.0), (1.0, 2.0, -49.0), _lam(0.0, 0.0, 0.0)))
    return _room_cfg(objs)


# ------------------------------------------------------------------ umbra and penumbra: a check without a restatement
# A floor y = 0, a thin panel at y = 4 (|x| <= 0.5, |z| <= PANEL_HALF_Z) and a black (albedo 0) occluder at y = 2 (|x|, |z| <= 1) under a
# black sky; the camera hangs below the occluder's height and looks down, so it sees floor only, and every ray scattered from the floor
# goes up (normal + a point of the open unit ball) to the occluder's underside, the panel or the sky.
# The segment from a floor point P to a panel point T crosses y = 2 at (P + T) / 2: it is blocked iff |Px + Tx| <= 2 and |Pz + Tz| <= 2.
#   umbra       no T visible:        |Px| + 0.5 <= 2 and |Pz| + PANEL_HALF_Z <= 2
#   inner band  the centre T = 0 is hidden and some T is visible:  1.5 < |Px| <= 2 (with |Pz| + PANEL_HALF_Z <= 2)
#   lit         every T visible:     |Px| - 0.5 > 2  (or |Pz| - PANEL_HALF_Z > 2)
# The panel is thin so that a SCATTERED ray practically never reaches it (solid angle / pi ~ 1e-4 per sample): what lights the inner band
# is the light loop's aim — a fresh point of the panel — and an aim at the centre leaves it black.
SHADOW_W, SHADOW_H, SHADOW_SPP = 48, 8, 64
PANEL_HALF_Z = 0.004
MARGIN = 1e-9


def shadow_cfg():
    objs = [_quad((-30, 0, -30), (60, 0, 0), (0, 0, 60), _lam(0.9, 0.9, 0.9)),
            emitting(_quad((-0.5, 4, -PANEL_HALF_Z), (1.0, 0, 0), (0, 0, 2 * PANEL_HALF_Z), WHITE), (1.0, 1.0, 1.0)),
            _quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), _lam(0.0, 0.0, 0.0))]
    return _cfg(objs, sky=False, look_from=(0.0, 1.5, 6.0), look_at=(0.0, 0.0, 0.0), vfov=10.0, aspect=6.0)


def footprints(c):
    """per pixel the floor points of its four corner rays, [H, W, 4, 2] (x, z) in f64: the jitter keeps a sample's ray inside them, the
    map from the image plane to the floor is projective and the regions below are convex or complements of slabs tested per corner"""
    org, ll, hor, ver = (np.array(list(v)) for v in (c.cam_origin, c.cam_lower_left, c.cam_horizontal, c.cam_vertical))
    Wd, Hd = c.width, c.height
    out = np.zeros((Hd, Wd, 4, 2))
    for y in range(Hd):
        for x in range(Wd):
            for i, (jx, jy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                u, v = (x + jx) / (Wd - 1.0), (Hd - (y + jy)) / (Hd - 1.0)
                d = ll + hor * u + ver * v - org
                assert d[1] < 0.0, "the camera must see floor only"
                t = -org[1] / d[1]
                out[y, x, i] = (org[0] + d[0] * t, org[2] + d[2] * t)
    return out


def check_shadow(c, rgb, lin):
    """the assertions of the umbra / penumbra check on a frame of shadow_cfg(); returns the figures it used"""
    fp = footprints(c)
    ax, az = np.abs(fp[..., 0]), np.abs(fp[..., 1])
    in_z = (az + PANEL_HALF_Z <= 2.0 - MARGIN).all(axis=2)
    umbra = (ax + 0.5 <= 2.0 - MARGIN).all(axis=2) & in_z
    inner = ((ax > 1.5 + MARGIN) & (ax <= 2.0 - MARGIN)).all(axis=2) & in_z
    one_side = np.sign(fp[..., 0]).min(axis=2) == np.sign(fp[..., 0]).max(axis=2)      # (|x| > c is two half planes: a footprint lies in ONE)
    inner &= one_side
    lit = (ax - 0.5 > 2.0 + MARGIN).all(axis=2) & one_side
    assert umbra.sum() >= 8 and inner.sum() >= 8 and lit.sum() >= 8, (int(umbra.sum()), int(inner.sum()), int(lit.sum()))
    assert (lin[umbra] == 0.0).all() and (rgb[umbra] == 0).all(), "light in the umbra"
    m_inner, m_lit = float(lin[inner].mean()), float(lin[lit].mean())
    # the inner band sees between none and half of the panel (a quarter on average), the lit floor all of it, and the estimator weighs a
    # light ray by neither distance nor angle: the band's mean is a quarter of the lit floor's, give or take the noise of a few hundred rays
    assert (lin[inner] > 0.0).any(), "the inner penumbra is black: the aim does not sample the panel"
    assert 0.0 < m_inner < 0.6 * m_lit, (m_inner, m_lit)
    some = lin[inner][(lin[inner] > 0.0).any(axis=1)]
    assert (some.max(axis=1) < lin[lit].max()).any()
    return {"umbra": int(umbra.sum()), "inner": int(inner.sum()), "lit": int(lit.sum()), "mean_inner": m_inner, "mean_lit": m_lit}
