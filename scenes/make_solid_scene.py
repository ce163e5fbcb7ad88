"""scenes/cover_solid_1200x800_spp128.json: the cover scene of scenes/cfg2_cover_1200x800_spp128.json with solid textures
(DESIGN.md §16): the ground (radius 1000) becomes a checker, the big Lambertian sphere (radius 1) a marble ball, and every sixth small
Lambertian sphere a Noise sphere, alternately in `noise` and `turbulence` mode.  Colours, scales and seeds are drawn from a fixed seed.

    python scenes/make_solid_scene.py        # rewrites the file (deterministic)"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cfg2_cover_1200x800_spp128.json")
OUT = os.path.join(HERE, "cover_solid_1200x800_spp128.json")
SEED = 20261018


def make():
    with open(SRC) as f:
        cfg = json.load(f)
    rng = np.random.default_rng(SEED)
    objects, big, small = [], False, 0
    for i, o in enumerate(cfg["objects"]):
        mat = o["material"]
        if i == 0:
            assert o["radius"] == 1000.0, "the cover scene's first sphere is its ground"
            mat = {"Checker": {"even": [0.9, 0.9, 0.9], "odd": [0.2, 0.3, 0.1], "scale": 1.0}}
        elif not big and "Lambertian" in mat and o["radius"] == 1.0:
            mat = {"Noise": {"albedo": [0.95, 0.93, 0.9], "scale": 3.0, "mode": "marble", "octaves": 7, "seed": int(rng.integers(1 << 32))}}
            big = True
        elif "Lambertian" in mat and o["radius"] == 0.2:
            if small % 6 == 0:
                mat = {"Noise": {"albedo": [round(float(v), 3) for v in rng.uniform(0.5, 1.0, 3)], "scale": round(float(rng.uniform(8.0, 20.0)), 2),
                                 "mode": ("noise", "turbulence")[small // 6 % 2], "octaves": int(rng.integers(2, 8)), "seed": int(rng.integers(1 << 32))}}
            small += 1
        objects.append({"center": o["center"], "radius": o["radius"], "material": mat})
    assert big and small >= 12, "the cover scene has one big Lambertian sphere and many small ones"
    cfg["objects"] = objects
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(make())
