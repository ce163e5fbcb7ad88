"""scenes/cornell_image_600x600_spp128.json: the room of scenes/make_bvh_scene.py with pictures —
scenes/data/earth.jpg as a poster on the back wall, a smooth Lambertian icosphere (subdivision 3, radial normals) whose vertices carry
equirectangular (s, t) of the same file — a globe — and a Metal box that shows scenes/data/moon.jpg on every face.  An image comes in
beside the material: "image" and "uvs" are object-level keys, the materials stay Lambertian and Metal.  The globe's (s, t) are one pair
per vertex, so the faces that straddle the date line run the whole map backwards across one face's width: seams are out of scope.

    python scenes/make_cornell_image_scene.py                       # rewrites the file (deterministic)
    python scenes/make_cornell_image_scene.py --plain --out x.json  # the same room without any "image" / "uvs" (benchmarks)"""
import argparse
import json
import math
import os

from make_bvh_scene import icosphere, room
from make_cornell_mesh_scene import _lam, _mesh, _pt

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cornell_image_600x600_spp128.json")
EARTH, MOON = "scenes/data/earth.jpg", "scenes/data/moon.jpg"


def globe(c, r, subdivision, mat):
    unit, _ = icosphere((0.0, 0.0, 0.0), 1.0, subdivision)
    obj = _mesh(*icosphere(c, r, subdivision), mat)
    obj["mesh"]["normals"] = [[round(float(x), 6) for x in v] for v in unit]
    # longitude from +z towards +x, latitude from the south pole: s in [0, 1], t in [0, 1]
    obj["mesh"]["uvs"] = [[round(math.atan2(v[0], v[2]) / (2.0 * math.pi) + 0.5, 6), round(math.asin(max(-1.0, min(1.0, v[1]))) / math.pi + 0.5, 6)]
                          for v in unit]
    obj["image"] = {"pixels": EARTH, "wrap": ["repeat", "clamp"]}
    return obj


def make(plain=False):
    objects = room()
    objects[4] = dict(objects[4], image={"pixels": EARTH, "wrap": "clamp"}, uvs=[[1.0, 0.0], [0.0, 0.0], [1.0, 1.0]])   # the back wall, seen from inside
    objects.append(globe((390.0, 120.0, 190.0), 110.0, 3, _lam(0.8, 0.8, 0.8)))
    objects.append({"box": {"min": [90.0, 0.0, 280.0], "max": [260.0, 250.0, 450.0]}, "material": {"Metal": {"albedo": [0.9, 0.9, 0.9], "fuzz": 0.15}},
                    "image": {"pixels": MOON}})
    if plain:
        for o in objects:
            o.pop("image", None)
            o.pop("uvs", None)
            if "mesh" in o:
                o["mesh"].pop("uvs", None)
    cfg = {"width": 600, "height": 600, "samples_per_pixel": 128, "max_depth": 50, "sky": None,
           "camera": {"look_from": _pt(278, 278, -800), "look_at": _pt(278, 278, 0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": 1.0},
           "objects": objects, "flat_bvh": True}
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", action="store_true", help="the room without its images")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(make(a.plain))
