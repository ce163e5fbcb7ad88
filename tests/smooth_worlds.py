"""Worlds and point tables the CPU and the GPU tests of shading normals share.  TEST INFRASTRUCTURE."""
import functools
import math

import numpy as np

from test_medium_gpu import _cfg, _lam, _med, _obj
from test_quad_gpu import GLASS, LENS_KEYS, _chk, _floor_objs, _metal

W, H, SPP = 48, 32, 4


@functools.lru_cache(maxsize=None)
def icosphere(level):
    """(vertices on the unit sphere, faces wound outward) of an icosahedron subdivided `level` times: 20 * 4^level faces"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]

    def unit(p):
        l = math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        return (p[0] / l, p[1] / l, p[2] / l)
    v = [unit(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                v.append(unit(tuple((v[a][k] + v[b][k]) / 2.0 for k in range(3))))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    for a, b, c in f:   # outward: cross(b - a, c - a) . a > 0
        u, w = [v[b][k] - v[a][k] for k in range(3)], [v[c][k] - v[a][k] for k in range(3)]
        n = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])
        assert n[0] * v[a][0] + n[1] * v[a][1] + n[2] * v[a][2] > 0.0
    return tuple(v), tuple(f)


def ico_mesh(level, centre, radius, mat, normals="radial", smooth=None):
    """a {"mesh": ...} object: the icosphere scaled and moved; normals: "radial" (the unit-sphere vertices), None, or a list"""
    v, f = icosphere(level)
    mesh = {"vertices": [[centre[k] + radius * p[k] for k in range(3)] for p in v], "faces": [list(t) for t in f]}
    if normals == "radial":
        mesh["normals"] = [list(p) for p in v]
    elif normals is not None:
        mesh["normals"] = normals
    if smooth is not None:
        mesh["smooth"] = smooth
    return {"mesh": mesh, "material": mat}


def strip_normals(cfg):
    """the same scene file without any `normals` / `smooth` key"""
    import copy
    cfg = copy.deepcopy(cfg)
    for o in cfg["objects"]:
        o.pop("normals", None)
        if "mesh" in o:
            o["mesh"].pop("normals", None); o["mesh"].pop("smooth", None)
    return cfg


PARITY_CASES = ["metal", "glass", "lambertian", "lens_moving_medium", "checker"]
PINHOLE_CASES = ["metal", "glass", "lambertian", "checker"]      # what tests/lanesim/ renders: no lens


def parity_cfg(case):
    """48 x 32 scenes with an icosphere carrying radial normals: the metal one (and its flat_bvh twin) the 320-face mesh, the others
    level 1 (80 faces: what the Python restatement renders in a few seconds each)"""
    if case == "metal":
        return _cfg(_floor_objs(extra=[ico_mesh(2, (-0.6, 0.9, 2.2), 0.9, _metal((0.9, 0.9, 0.95), 0.0))]))   # the 320-face mesh
    if case == "glass":   # every third vertex normal is swung far round the y axis: some hits' interpolated normal points through its face
        v, _ = icosphere(1)
        swung = [list(p) if i % 3 else [p[0] + 6.0 * p[2], p[1], p[2] - 6.0 * p[0]] for i, p in enumerate(v)]
        return _cfg(_floor_objs(extra=[ico_mesh(1, (-0.4, 0.8, 2.4), 1.0, GLASS, normals=swung)]))
    if case == "lambertian":
        return _cfg(_floor_objs(extra=[ico_mesh(1, (-0.6, 0.9, 2.2), 0.9, _lam(0.3, 0.7, 0.4))]))
    if case == "lens_moving_medium":
        return _cfg(_floor_objs(True, extra=[_obj((-1.0, 0.6, -2.2), 0.9, _med((0.9, 0.6, 0.3), 2.0)), ico_mesh(1, (-0.6, 0.9, 2.2), 0.9, _lam(0.3, 0.7, 0.4))]),
                    lens=LENS_KEYS)
    if case == "checker":
        return _cfg(_floor_objs(extra=[ico_mesh(1, (-0.6, 0.9, 2.2), 0.9, _chk((0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 0.4))]))
    raise KeyError(case)


def box_triangles(mn, mx, mat, with_normals):
    """an axis-aligned box as 12 {"triangle": ...} objects wound outward, each (with_normals) carrying its face's +- axis three times"""
    x0, y0, z0 = mn
    x1, y1, z1 = mx
    faces = [((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), (1, 0, 0)), ((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), (-1, 0, 0)),
             ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (0, 1, 0)), ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), (0, -1, 0)),
             ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (0, 0, 1)), ((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), (0, 0, -1))]
    out = []
    for a, b, c, d, n in faces:
        for tri in ((a, b, c), (a, c, d)):
            o = {"triangle": [[float(x) for x in p] for p in tri], "material": mat}
            if with_normals:
                o["normals"] = [[float(x) for x in n]] * 3
            out.append(o)
    return out


def box_cfg(with_normals, mat=None):
    return _cfg(_floor_objs(extra=box_triangles((-1.5, -0.5, 1.6), (-0.25, 0.75, 2.85), mat or _metal((0.9, 0.8, 0.7), 0.0), with_normals)))


def sphere_limit_cfg():
    """a level-2 icosphere (320 faces) ON the unit sphere at the origin, normals = vertices, alone under the sky"""
    return _cfg([ico_mesh(2, (0.0, 0.0, 0.0), 1.0, _lam(0.7, 0.6, 0.5))], look_from=(0.3, 0.4, 3.2), look_at=(0.0, 0.0, 0.0), vfov=45.0)


def file_normals(host_scene):
    """the [n_quads, 9] array of a loaded scene, zeros where the file has none"""
    n = host_scene.flat_normals()
    q = host_scene.quads()
    return n if n is not None else np.zeros((len(q), 9))
