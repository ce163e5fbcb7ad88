"""scenes/cornell_flat_motion_600x600_spp128.json: the room of scenes/make_bvh_scene.py in which a box falls and a small smooth icosphere
slides while the shutter is open: "move": [dx, dy, dz] on the box and on the mesh, the displacement over the open shutter.
Both blur; the room stays sharp.  Generated, not committed (53 KB with the default subdivision).

    python scenes/make_flat_motion_scene.py                                     # rewrites the file (deterministic)
    python scenes/make_flat_motion_scene.py --subdivision 1 --out DIR/x.json    # a smaller icosphere (tests)
    python scenes/make_flat_motion_scene.py --still                             # the same room with nothing moving"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_bvh_scene import METAL, room  # noqa: E402
from make_cornell_mesh_scene import _pt  # noqa: E402
from make_smooth_scene import smooth_icosphere  # noqa: E402

OUT = os.path.join(HERE, "cornell_flat_motion_600x600_spp128.json")
WHITE = {"Lambertian": {"albedo": [0.73, 0.73, 0.73]}}


def make(subdivision=None, still=False):
    box = {"box": {"min": [265.0, 150.0, 295.0], "max": [430.0, 315.0, 460.0]}, "material": WHITE}
    ball = smooth_icosphere((170.0, 70.0, 170.0), 70.0, 3 if subdivision is None else subdivision, METAL)
    if not still:
        box["move"] = [0.0, -90.0, 0.0]       # falling
        ball["move"] = [110.0, 0.0, 30.0]     # sliding along the floor
    cfg = {"width": 600, "height": 600, "samples_per_pixel": 128, "max_depth": 50, "sky": None,
           "camera": {"look_from": _pt(278, 278, -800), "look_at": _pt(278, 278, 0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": 1.0},
           "objects": room() + [box, ball], "flat_bvh": True}
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivision", type=int, default=None, help="the icosphere at this subdivision instead of the example's 3")
    ap.add_argument("--still", action="store_true", help="write the room without any \"move\"")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(make(a.subdivision, a.still))
