"""The worlds of the sphere-update tests (tests/test_update_gpu.py, tests/test_update_cpu.py): a scene as JSON text, its centres,
and the centres an update moves them to.  TEST INFRASTRUCTURE."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 64, 48, 3, 8


def _lamb(rng):
    return {"Lambertian": {"albedo": [round(float(v), 3) for v in rng.uniform(0.1, 0.9, 3)]}}


def _mat(rng, i):
    return _lamb(rng) if i % 5 else ({"Metal": {"albedo": [0.8, 0.7, 0.6], "fuzz": 0.1}} if i % 2 else {"Glass": {"index_of_refraction": 1.5}})


def _obj(c, r, m):
    return {"center": {"x": float(c[0]), "y": float(c[1]), "z": float(c[2])}, "radius": float(r), "material": m}


def _cfg(objs, look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), vfov=25.0):
    return {"width": W, "height": H, "samples_per_pixel": SPP, "max_depth": DEPTH, "sky": {"texture": ""},
            "camera": {"look_from": dict(zip("xyz", look_from)), "look_at": dict(zip("xyz", look_at)), "vup": {"x": 0.0, "y": 1.0, "z": 0.0},
                       "vfov": vfov, "aspect": W / H}, "objects": objs}


def centres_of(cfg):
    return np.array([[o["center"][k] for k in "xyz"] for o in cfg["objects"]], np.float64)


def set_centres(abi, sc, c):
    """write n x 3 centres into the RtSphere records of a loaded scene (NaN and inf included: no JSON carries those)"""
    n = sc.c.n_spheres
    words = C.sizeof(abi.RtSphere) // 8
    raw = (C.c_double * (words * n)).from_address(C.addressof(sc.c.spheres.contents))
    np.frombuffer(raw, np.float64).reshape(n, words)[:, :3] = np.asarray(c, np.float64).reshape(n, 3)


class World:
    def __init__(self, cfg, steps, expect=None, env=None, **extra):
        self.text = json.dumps(cfg)
        self.base = centres_of(cfg)
        self.steps = steps                    # [(center, center1 or None)]
        self.expect = expect or [{} for _ in steps]
        self.env = env or {}
        self.__dict__.update(extra)


def _lattice(rng, half=11):
    """the cover scene's layout: a ground ball, three unit balls, a jittered lattice of small ones (488 spheres at half = 11)"""
    objs = [_obj((0, -1000, 0), 1000, {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}), _obj((0, 1, 0), 1.0, {"Glass": {"index_of_refraction": 1.5}}),
            _obj((-4, 1, 0), 1.0, {"Lambertian": {"albedo": [0.4, 0.2, 0.1]}}), _obj((4, 1, 0), 1.0, {"Metal": {"albedo": [0.7, 0.6, 0.5], "fuzz": 0.0}})]
    for a in range(-half, half):
        for b in range(-half, half):
            objs.append(_obj((a + 0.9 * rng.random(), 0.2, b + 0.9 * rng.random()), 0.2, _mat(rng, len(objs))))
    return objs


def _few(rng, n, light=None):
    objs = [_obj(rng.uniform(-3, 3, 3), rng.uniform(0.2, 0.5), _mat(rng, i)) for i in range(n)]
    if light is not None:
        objs[light]["material"] = {"Light": {}}
    return objs


def _spheres30(rng):
    cfg = _cfg(_few(rng, 30))
    c = centres_of(cfg)
    return World(cfg, [(c + rng.uniform(-0.5, 0.5, c.shape), None)], [{"grid_cells": lambda v: v > 0, "grid_large": lambda v: v < 30}])


def _all_large_and_back(rng):
    cfg = _cfg(_few(rng, 24))
    c = centres_of(cfg)
    bad = c + rng.uniform(-0.2, 0.2, c.shape)
    bad[7, 1] = np.nan                      # 23 gridded spheres: below min_spheres, the grid disappears
    back = c + rng.uniform(-0.2, 0.2, c.shape)
    return World(cfg, [(bad, None), (back, None)], [{"grid_cells": 0, "grid_large": 24}, {"grid_cells": lambda v: v > 0}])


def _lattice488(rng):
    cfg = _cfg(_lattice(rng))
    c = centres_of(cfg)
    assert len(c) == 488
    moved = c.copy()
    moved[4:] += rng.uniform(-0.4, 0.4, (484, 3)) * np.array([1.0, 0.0, 1.0])
    return World(cfg, [(moved, None)], [{"grid_cells": lambda v: v > 500, "grid_large": 4, "grid_wide": 0}])


def _procedural(rng):
    sys.path.insert(0, os.path.join(ROOT, "scenes"))
    import procedural
    cfg = procedural.make_config(width=W, height=H, spp=2, max_depth=DEPTH, half=50)
    c = centres_of(cfg)
    moved = c.copy()
    small = np.array([abs(o["radius"]) < 0.5 for o in cfg["objects"]])
    moved[small] += rng.uniform(-0.2, 0.2, (int(small.sum()), 3)) * np.array([1.0, 0.0, 1.0])
    return World(cfg, [(moved, None)], [{"n_spheres": lambda v: v > 9000, "grid_cells": lambda v: v > 50000, "grid_wide": 0}])   # (the scan crosses many workgroups)


def _cluster(rng):
    objs = [_obj(rng.uniform(-10, 10, 3) * np.array([1, 0.05, 1]), 0.1, _mat(rng, i)) for i in range(150)]
    objs += [_obj(np.array([1.0, 0.0, 1.0]) + rng.uniform(-0.5, 0.5, 3), 0.08, _mat(rng, i)) for i in range(400)]
    cfg = _cfg(objs)
    c = centres_of(cfg)
    moved = c.copy()
    moved[150:] = np.array([2.0, 0.0, -1.0]) + rng.uniform(-0.02, 0.02, (400, 3))   # centres inside one cell's width: long lists
    return World(cfg, [(moved, None)], [{"grid_items": lambda v: v > 400, "grid_wide": 0}])


def _demote(rng):
    objs = [_obj((a + 0.5, 0.1, b + 0.5), 0.1, _mat(rng, a * 20 + b)) for a in range(-10, 10) for b in range(-10, 10)]
    objs.append(_obj((0.0, 0.39, 0.0), 0.39, {"Metal": {"albedo": [0.9, 0.9, 0.9], "fuzz": 0.0}}))   # below 4 x the median radius: gridded
    cfg = _cfg(objs)
    c = centres_of(cfg)
    moved = c.copy()
    moved[:400, 0] *= 0.05                   # the lattice closes in around the last sphere: cells shrink, it covers more than 512
    moved[:400, 2] *= 0.05
    return World(cfg, [(c + 0.0, None), (moved, None)], [{"grid_large": 0}, {"grid_large": lambda v: v >= 1, "grid_cells": lambda v: v > 0}])


def _moving(rng):
    cfg = _cfg(_lattice(rng))
    c = centres_of(cfg)
    moved = c.copy()
    moved[4:] += rng.uniform(-0.3, 0.3, (484, 3)) * np.array([1.0, 0.0, 1.0])
    c1 = moved.copy()
    c1[4::3] += rng.uniform(-0.3, 0.3, c1[4::3].shape) * np.array([1.0, 0.5, 1.0])   # every third small sphere moves over the shutter
    c1[2] += np.array([0.0, 0.4, 0.0])                                               # and a unit ball, one of the `large` list
    return World(cfg, [(moved, c1)], [{"motion": lambda v: v > 100, "grid_cells": lambda v: v > 500}])


def _crowd(rng, n_crowd=5000, medium=False):
    objs = [_obj((0, -1000, 0), 1000, {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}})]
    xs, zs = rng.uniform(-8, 8, n_crowd + 300), rng.uniform(-8, 8, n_crowd + 300)
    for i in range(n_crowd + 300):
        objs.append(_obj((xs[i], 0.02, zs[i]), 0.02, _mat(rng, i)))
    if medium:
        objs[5]["material"] = {"Medium": {"albedo": [0.5, 0.5, 0.5], "density": 2.0}}
    cfg = _cfg(objs, look_from=(6.0, 1.5, 2.0), vfov=30.0)
    c = centres_of(cfg)
    moved = c.copy()
    moved[1:1 + n_crowd] = np.array([0.5, 0.02, 0.5])      # coincident: one cell holds more than 4 095 items
    return World(cfg, [(c + 0.0, None), (moved, None)], [{"grid_wide": 0}, {"grid_wide": 1, "grid_cells": lambda v: v > 0}])


def _wide300(rng):
    cfg = _cfg(_few(rng, 300))
    c = centres_of(cfg)
    return World(cfg, [(c + rng.uniform(-0.5, 0.5, c.shape), None)], [{"grid_wide": 1, "grid_cells": lambda v: v > 0}], env={"RT_GRID_WIDE": "1"})


def _lit30(rng):
    return World(_cfg(_few(rng, 30, light=3)), [], light=3)


WORLDS = {"spheres30": _spheres30, "all_large_and_back": _all_large_and_back, "lattice488": _lattice488, "procedural10004": _procedural,
          "cluster": _cluster, "demote": _demote, "moving": _moving, "crowd5000": _crowd, "wide300": _wide300}
OTHER = {"lit30": _lit30, "medium_crowd": lambda rng: _crowd(rng, 4300, medium=True)}


def make_world(name):
    maker = WORLDS.get(name) or OTHER[name]
    return maker(np.random.default_rng(sorted(list(WORLDS) + list(OTHER)).index(name) + 40))
