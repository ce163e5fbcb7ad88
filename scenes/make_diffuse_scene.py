"""scenes/cover_diffuse_1200x800_spp128.json: the cover scene of scenes/cfg2_cover_1200x800_spp128.json with every Metal and Glass sphere
made Lambertian — a Metal sphere keeps its albedo, a Glass sphere gets an albedo drawn from a fixed seed.  No mirror and no lens is left:
the scene temporal denoising is measured on where first-hit reprojection has nothing it cannot follow.

    python scenes/make_diffuse_scene.py        # rewrites the file (deterministic)"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cfg2_cover_1200x800_spp128.json")
OUT = os.path.join(HERE, "cover_diffuse_1200x800_spp128.json")
SEED = 20261018


def make():
    with open(SRC) as f:
        cfg = json.load(f)
    rng = np.random.default_rng(SEED)
    objects, changed = [], 0
    for o in cfg["objects"]:
        mat = o["material"]
        if "Metal" in mat:
            mat = {"Lambertian": {"albedo": mat["Metal"]["albedo"]}}
            changed += 1
        elif "Glass" in mat:
            mat = {"Lambertian": {"albedo": [round(float(v), 3) for v in rng.uniform(0.3, 0.9, 3)]}}
            changed += 1
        objects.append({"center": o["center"], "radius": o["radius"], "material": mat})
    assert changed >= 20, "the cover scene has many Metal and Glass spheres"
    cfg["objects"] = objects
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(make())
