"""scenes/cover_motion_1200x800_spp128.json: the cover scene of scenes/cfg2_cover_1200x800_spp128.json with its small diffuse spheres
bouncing, the first image of "The Next Week" (motion blur).  Every Lambertian sphere of radius 0.2 gets
center1 = center + (0, U[0, 0.5), 0), drawn in object order from a fixed seed; every other sphere stays static.

    python scenes/make_motion_scene.py        # rewrites the file (deterministic)"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cfg2_cover_1200x800_spp128.json")
OUT = os.path.join(HERE, "cover_motion_1200x800_spp128.json")
SEED = 20260914


def make():
    with open(SRC) as f:
        cfg = json.load(f)
    rng = np.random.default_rng(SEED)
    objects = []
    for o in cfg["objects"]:
        if "Lambertian" in o["material"] and o["radius"] == 0.2:
            c = o["center"]
            c1 = {"x": c["x"], "y": c["y"] + float(rng.uniform(0.0, 0.5)), "z": c["z"]}
            o = {"center": c, "center1": c1, "radius": o["radius"], "material": o["material"]}
        objects.append(o)
    cfg["objects"] = objects
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(make())
