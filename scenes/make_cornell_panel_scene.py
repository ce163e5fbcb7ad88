"""scenes/cornell_panel_600x600_spp128.json: the Cornell-box-like room of scenes/make_cornell_scene.py with the sphere lamp
replaced by the canonical ceiling panel — a quad just under the ceiling that emits (`"emit": [1.0, 0.9, 0.75]`) and is
SAMPLED: every light ray aims at a fresh point of the panel, so the boxes and the balls cast penumbrae.  Black sky, max_depth 50:
everything the frame shows is lit by the panel.  The room is 555 units wide, as the book's; the panel is the book's 130 x 105.

    python scenes/make_cornell_panel_scene.py        # rewrites the file (deterministic)"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cornell_panel_600x600_spp128.json")


def _pt(x, y, z):
    return {"x": float(x), "y": float(y), "z": float(z)}


def _quad(q, u, v, mat):
    return {"q": _pt(*q), "u": _pt(*u), "v": _pt(*v), "material": mat}


def _lam(r, g, b):
    return {"Lambertian": {"albedo": [r, g, b]}}


def make():
    white, red, green = _lam(0.73, 0.73, 0.73), _lam(0.65, 0.05, 0.05), _lam(0.12, 0.45, 0.15)
    objects = [
        _quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green),          # right
        _quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),              # left
        _quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white),            # floor
        _quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white),    # ceiling
        _quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white),          # back
        dict(_quad((213, 554, 227), (130, 0, 0), (0, 0, 105), white), emit=[1.0, 0.9, 0.75]),   # the ceiling panel
        {"box": {"min": [265.0, 0.0, 295.0], "max": [430.0, 330.0, 460.0]}, "material": white},   # the tall box
        {"box": {"min": [130.0, 0.0, 65.0], "max": [295.0, 165.0, 230.0]}, "material": white},    # the short box
        {"center": _pt(212, 225, 147), "radius": 60.0, "material": {"Glass": {"index_of_refraction": 1.5}}},
        {"center": _pt(440, 70, 150), "radius": 70.0, "material": {"Metal": {"albedo": [0.9, 0.9, 0.9], "fuzz": 0.0}}},
    ]
    cfg = {"width": 600, "height": 600, "samples_per_pixel": 128, "max_depth": 50, "sky": None,
           "camera": {"look_from": _pt(278, 278, -800), "look_at": _pt(278, 278, 0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": 1.0},
           "objects": objects}
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(make())
