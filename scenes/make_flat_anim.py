"""An animated mesh for `raytracer --frames N --flat-frames PREFIX`: a base scene file and N frame files of a small
rippling heightfield — a Metal sheet of 2 n^2 triangles over a Lambertian ground, two spheres beside it.  Frame f's file is the base
file with the sheet's vertices at phase 2 pi f / N; the CLI takes only the flat primitives of a frame file, so count, shapes and
materials are the base file's by construction.  The files are written, not committed (scenes/flat_anim/ by default).

    python scenes/make_flat_anim.py                       # scenes/flat_anim/flat_anim.json + flat_anim_000.json .. _007.json
    python scenes/make_flat_anim.py --n 64 --frames 32 --out DIR --width 600 --height 400 --spp 64
    raytracer scenes/flat_anim/flat_anim.json out/frame --frames 8 --orbit 0 --flat-frames scenes/flat_anim/flat_anim_"""
import argparse
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _pt(x, y, z):
    return {"x": float(x), "y": float(y), "z": float(z)}


def sheet(n, size, phase):
    """(vertices, faces) of an n x n grid of cells over [-size/2, size/2]^2, two triangles a cell, wound so that the normals point up"""
    xs = [-size / 2.0 + size * i / n for i in range(n + 1)]

    def height(x, z):
        return 0.9 + 0.22 * math.sin(1.6 * x + phase) * math.cos(1.1 * z - 0.5 * phase) + 0.08 * math.sin(2.7 * (x + z) + 2.0 * phase)
    verts = [[round(x, 4), round(height(x, z), 4), round(z, 4)] for x in xs for z in xs]
    at = lambda i, j: i * (n + 1) + j
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            faces += [[a, c, b], [a, d, c]]
    return verts, faces


def make(n=24, phase=0.0, width=300, height=200, spp=16):
    verts, faces = sheet(n, 6.0, phase)
    objects = [
        {"center": _pt(0, -1000, 0), "radius": 1000.0, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}},
        {"center": _pt(-2.2, 2.1, 0.4), "radius": 0.6, "material": {"Lambertian": {"albedo": [0.8, 0.3, 0.2]}}},
        {"center": _pt(1.9, 2.0, -1.2), "radius": 0.5, "material": {"Glass": {"index_of_refraction": 1.5}}},
        {"mesh": {"vertices": verts, "faces": faces}, "material": {"Metal": {"albedo": [0.8, 0.85, 0.9], "fuzz": 0.02}}},
    ]
    cfg = {"width": width, "height": height, "samples_per_pixel": spp, "max_depth": 16, "sky": {"texture": ""},
           "camera": {"look_from": _pt(0.0, 5.5, 8.0), "look_at": _pt(0.0, 0.8, 0.0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": width / height},
           "objects": objects, "flat_bvh": True}
    return json.dumps(cfg, separators=(",", ":"))


def write(out_dir, n=24, frames=8, **kw):
    """writes the base file and the frame files -> (base path, the prefix to give --flat-frames)"""
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, "flat_anim.json")
    with open(base, "w") as f:
        f.write(make(n, 0.0, **kw))
    prefix = os.path.join(out_dir, "flat_anim_")
    for k in range(frames):
        with open(f"{prefix}{k:03d}.json", "w") as f:
            f.write(make(n, 2.0 * math.pi * k / frames, **kw))
    return base, prefix


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24, help="cells along each side: 2 n^2 triangles")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "flat_anim"))
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--height", type=int, default=200)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    print(*write(a.out, a.n, a.frames, width=a.width, height=a.height, spp=a.spp))
