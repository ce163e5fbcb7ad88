"""The worlds of the parity frames of flat primitives that move within the frame and the restatement's frames of them,
computed once per session and left unchanged: the CPU and the GPU tests share them.  TEST INFRASTRUCTURE."""
import copy

import numpy as np

import flat_motion_mini as FM
import smooth_worlds as SW
from test_medium_gpu import _cfg, _lam, _load, _med, _obj
from test_quad_gpu import GLASS, LENS_KEYS, _box, _chk, _floor_objs, _metal, _noi, _quad, _room_objs

W, H, SPP, DEPTH = 48, 32, 4, 8
PARITY_CASES = ["room_box", "glass_pane", "mirror", "solids", "smooth_mesh", "lens_spheres_medium", "flat_only"]
CPU_CASES = [c for c in PARITY_CASES if "lens" not in c]       # what tests/lanesim/ renders: every case without a lens, the lit room included
_CACHE = {}


def _moved(o, m):
    o = copy.deepcopy(o)
    o["move"] = [float(x) for x in m]
    return o


def parity_cfg(case):
    """48 x 32 scenes written with "move" in the file, so that the loader's table is what the scene is given"""
    if case == "room_box":              # the lit room; its box falls
        objs = _room_objs()
        objs[6] = _moved(_box((-1.3, -0.2, -1.2), (-0.3, 1.4, -0.2), _lam(0.73, 0.73, 0.73)), (0.0, -0.8, 0.0))
        return _cfg(objs, sky=False, look_from=(0.0, 1.0, 7.0), look_at=(0.0, 0.8, 0.0))
    if case == "glass_pane":            # a Glass pane slides in front of the spheres
        return _cfg(_floor_objs(extra=[_moved(_quad((-1.8, -0.4, 3.0), (2.2, 0, 0.3), (0, 1.8, 0), GLASS), (1.2, 0.1, 0.0))]))
    if case == "mirror":                # a mirror quad swings back
        return _cfg(_floor_objs(extra=[_moved(_quad((-3.0, -0.5, 1.0), (1.5, 0, 1.5), (0, 2.2, 0), _metal((0.95, 0.95, 0.95), 0.0)), (0.3, 0.0, -0.9))]))
    if case == "solids":                # a Checker floor tile and a Noise wall move: the patterns ride
        return _cfg(_floor_objs(extra=[_moved(_quad((-1.5, -0.45, 2.0), (2.0, 0, 0), (0, 0, 1.6), _chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 0.35)), (0.9, 0.0, 0.2)),
                                       _moved(_quad((1.2, -0.5, -1.0), (0.4, 0, 2.4), (0, 2.0, 0), _noi((0.8, 0.7, 0.5), 3.0, "marble", 4, 7)), (0.0, 0.5, 0.4))]))
    if case == "smooth_mesh":           # a smooth-shaded icosphere slides
        return _cfg(_floor_objs(extra=[_moved(SW.ico_mesh(1, (-0.6, 0.9, 2.2), 0.9, _metal((0.9, 0.9, 0.95), 0.0)), (0.7, -0.2, 0.3))]))
    if case == "lens_spheres_medium":   # moving flat primitives + moving spheres + a lens + a medium
        return _cfg(_floor_objs(True, extra=[_obj((-1.0, 0.6, -2.2), 0.9, _med((0.9, 0.6, 0.3), 2.0)),
                                             _moved(_box((-1.6, -0.5, 1.6), (-0.8, 0.3, 2.4), _lam(0.3, 0.7, 0.4)), (0.5, 0.6, 0.0)),
                                             _moved({"triangle": [[1.0, -0.5, 2.6], [2.0, -0.5, 2.2], [1.5, 0.8, 2.4]], "material": _metal((0.9, 0.7, 0.4), 0.1)}, (-0.4, 0.2, 0.3))]),
                    lens=LENS_KEYS)
    if case == "flat_only":             # the only mover is a flat primitive; the floor quad moves too, within its own plane
        objs = _floor_objs()
        objs[0] = _moved(objs[0], (0.5, 0.0, -0.25))
        objs[3] = _moved(objs[3], (0.0, 0.4, 0.6))
        return _cfg(objs)
    raise KeyError(case)


def world(host, case):
    """(host scene, center1, lens, quads, normals [n, 9] or None, move [n, 3]) of one parity case"""
    sc, c1, lens = _load(host, parity_cfg(case), W, H, SPP, DEPTH, seed=131)
    move = sc.flat_motion()
    assert move is not None and (move != 0).any() and (lens is not None) == ("lens" in case) and (c1 is not None) == ("spheres" in case)
    return sc, c1, lens, sc.quads(), sc.flat_normals(), move


def mini(oracle, abi, sc, c1, lens, quads, normals, move):
    L = oracle.lib(abi)
    return FM.FlatMotionMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), c1, lens, quads, normals, move)


def mini_frame(oracle, abi, host, case):
    if case not in _CACHE:
        sc, c1, lens, quads, normals, move = world(host, case)
        m = mini(oracle, abi, sc, c1, lens, quads, normals, move)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _CACHE[case] = {"rgb": rgb, "lin": lin, "segments": segs, "discarded": m.discarded}
    return _CACHE[case]


def many_triangles(n=1100, seed=77):
    """(quv [n, 9], move [n, 3]) of n small triangles scattered over the floor of parity_cfg's view — past the scan's cap of 1024 — every other
    one moving"""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(-0.4, 1.6, n), rng.uniform(-2.0, 3.0, n)], axis=1)
    quv = np.concatenate([q, rng.uniform(-0.35, 0.35, (n, 3)), rng.uniform(-0.35, 0.35, (n, 3))], axis=1)
    move = np.zeros((n, 3))
    move[::2] = rng.uniform(-0.5, 0.5, (len(move[::2]), 3))
    return quv, move
