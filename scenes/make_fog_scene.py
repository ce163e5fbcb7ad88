"""scenes/cover_fog_1200x800_spp128.json: the cover scene of scenes/cfg2_cover_1200x800_spp128.json with participating media
(DESIGN.md §15): the big Lambertian sphere (radius 1) becomes a ball of smoke, and a thin haze sphere encloses the scene and the
camera (it lands in the `large` list, and every camera ray starts inside a medium).  The smoke's albedo and the two densities are
drawn from a fixed seed.

    python scenes/make_fog_scene.py        # rewrites the file (deterministic)"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cfg2_cover_1200x800_spp128.json")
OUT = os.path.join(HERE, "cover_fog_1200x800_spp128.json")
SEED = 20261017


def make():
    with open(SRC) as f:
        cfg = json.load(f)
    rng = np.random.default_rng(SEED)
    smoke = {"albedo": [round(float(v), 3) for v in rng.uniform(0.05, 0.15, 3)], "density": round(float(rng.uniform(2.0, 4.0)), 3)}
    haze = {"albedo": [0.9, 0.9, 0.95], "density": round(float(rng.uniform(0.008, 0.012)), 4)}
    objects, done = [], False
    for o in cfg["objects"]:
        if not done and "Lambertian" in o["material"] and o["radius"] == 1.0:
            o = {"center": o["center"], "radius": o["radius"], "material": {"Medium": smoke}}
            done = True
        objects.append(o)
    assert done, "the cover scene has one big Lambertian sphere"
    objects.append({"center": {"x": 0.0, "y": 0.0, "z": 0.0}, "radius": 60.0, "material": {"Medium": haze}})
    cfg["objects"] = objects
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(make())
