"""Scenes with a thin lens and / or moving spheres as the oracle and a resident scene take them:
shared by tests/test_oracle_lens_motion.py, tests/test_lens_motion_full_size.py, tests/golden/make_golden.py and tools/fuzz/gpu_fuzz.py."""
import ctypes as C
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")
TEST = os.path.join(ROOT, "scenes", "cfg1_test_800x600_spp16.json")
TEX = os.path.join(ROOT, "scenes", "cfg3_cover_4k_textured.json")
DOF = os.path.join(ROOT, "scenes", "cover_dof_1200x800_spp128.json")
MOTION_SCENE = os.path.join(ROOT, "scenes", "cover_motion_1200x800_spp128.json")
LENS, MOTION, LDS = 32, 64, 1   # bits of rt_hip_scene_query("last_kernel")


def config(path):
    with open(path) as f:
        return json.load(f)


def load(host, cfg, w=None, h=None, spp=None, depth=None, seed=None):
    """a scene config (a dict, or a path) -> (host scene, center1 or None, lens (u, v, r) or None).  With an "aperture" in the camera
    map the scene's camera fields are rt_camera_derive_lens's (on the focus plane), what rt_hip_set_camera takes beside
    rt_hip_set_lens; center1 is host.Scene.center1()'s list (None when no sphere has the key)."""
    if not isinstance(cfg, dict):
        cfg = config(cfg)
    sc = host.Scene.loads(json.dumps(cfg))
    c = sc.c
    if w:
        c.width = w
    if h:
        c.height = h
    if spp:
        c.samples_per_pixel = spp
    if depth is not None:
        c.max_depth = depth
    if seed is not None:
        c.seed = seed
    lens = None
    cam = cfg["camera"]
    if isinstance(cam, dict) and cam.get("aperture"):
        out = (C.c_double * 2)()
        host.lib().rt_scene_lens(sc._h, out)
        pt = lambda p: (float(p["x"]), float(p["y"]), float(p["z"]))
        d = host.camera_derive_lens(pt(cam["look_from"]), pt(cam["look_at"]), pt(cam["vup"]), float(cam["vfov"]), float(cam["aspect"]), out[0], out[1])
        for i in range(3):
            c.cam_origin[i], c.cam_lower_left[i], c.cam_horizontal[i], c.cam_vertical[i] = (d["origin"][i], d["lower_left_corner"][i],
                                                                                             d["horizontal"][i], d["vertical"][i])
        lens = (d["u"], d["v"], d["lens_radius"])
    return sc, sc.center1(), lens


def centres(sc):
    """the scene's own centres, n x 3 (a center1 that moves nothing)"""
    return np.array([[sc.c.spheres[i].center[k] for k in range(3)] for i in range(sc.c.n_spheres)], np.float64)


def move_some(abi, sc, rng, kind, frac=0.75):
    """center1 (n x 3) for a loaded scene: a seeded subset of its non-light spheres moves — along one axis ("axis"), diagonally
    ("diag") or across many cells ("long"), as tests/test_motion.py's _world_motion moves the adversarial worlds.  Spheres whose
    centre or radius is not finite stay where they are (center1 - center has to be finite)."""
    c0 = centres(sc)
    c1 = c0.copy()
    for i in range(sc.c.n_spheres):
        s = sc.c.spheres[i]
        go = rng.random() < frac          # (drawn for every sphere, so that the choice does not depend on the kinds)
        if kind == "axis":
            off = np.zeros(3); off[i % 3] = rng.uniform(-1.0, 1.0)
        elif kind == "diag":
            off = rng.uniform(-0.7, 0.7, 3)
        else:
            off = rng.uniform(-1.0, 1.0, 3); off *= rng.uniform(2.0, 8.0) / np.linalg.norm(off)
        if go and s.kind != abi.RT_MAT_LIGHT and np.isfinite(c0[i]).all() and abs(c0[i]).max() < 1e6:
            c1[i] = c0[i] + off
    return c1

