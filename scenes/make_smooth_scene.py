"""scenes/cornell_smooth_600x600_spp128.json: the room of scenes/make_bvh_scene.py — a Glass icosphere of 5 120 faces and a Metal one of
1 280 — with every vertex carrying its radial normal: "normals" inside each {"mesh": ...}, one [x, y, z] per vertex, the
vertex's direction from the sphere's centre.  The faces interpolate them, and the two polyhedra of the §22 example render as spheres.
Like that example the file is generated, not committed (the same size).

    python scenes/make_smooth_scene.py                                     # rewrites the file (deterministic)
    python scenes/make_smooth_scene.py --subdivision 2 --out DIR/x.json    # smaller icospheres (tests)"""
import argparse
import json
import os

from make_bvh_scene import GLASS, METAL, icosphere, room
from make_cornell_mesh_scene import _mesh, _pt

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cornell_smooth_600x600_spp128.json")


def smooth_icosphere(c, r, subdivision, mat):
    """the icosphere as a mesh object with one radial normal per vertex (six decimals; the loader keeps them as written, the library
    normalises them once)"""
    unit, _ = icosphere((0.0, 0.0, 0.0), 1.0, subdivision)
    obj = _mesh(*icosphere(c, r, subdivision), mat)
    obj["mesh"]["normals"] = [[round(float(x), 6) for x in v] for v in unit]
    return obj


def make(subdivision=None):
    glass, metal = (4, 3) if subdivision is None else (subdivision, subdivision)
    models = [smooth_icosphere((390.0, 110.0, 170.0), 105.0, glass, GLASS), smooth_icosphere((190.0, 125.0, 380.0), 120.0, metal, METAL)]
    cfg = {"width": 600, "height": 600, "samples_per_pixel": 128, "max_depth": 50, "sky": None,
           "camera": {"look_from": _pt(278, 278, -800), "look_at": _pt(278, 278, 0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": 1.0},
           "objects": room() + models, "flat_bvh": True}
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivision", type=int, default=None, help="both icospheres at this subdivision instead of the example's 4 and 3")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(make(a.subdivision))
