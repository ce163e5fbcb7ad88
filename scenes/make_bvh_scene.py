"""scenes/cornell_icosphere_600x600_spp128.json: the room of scenes/make_cornell_mesh_scene.py holding two models instead of three gems —
a Glass icosphere at subdivision 4 (5 120 faces) and a Metal one at subdivision 3 (1 280 faces), each a {"mesh": ...} object wound
outward — 6 400 triangles beside the five wall quads, and the top-level "flat_bvh": true that asks for the structure over them
(DESIGN.md §22): without it a file of more than 1 024 flat primitives is refused.  Vertices are printed with three decimals.

    python scenes/make_bvh_scene.py                                  # rewrites the file (deterministic)
    python scenes/make_bvh_scene.py --subdivision 6 --out DIR/x.json # ONE Metal icosphere of that subdivision in the room (benchmarks)"""
import argparse
import json
import os

from make_cornell_mesh_scene import _lam, _mesh, _pt, _quad, icosahedron

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cornell_icosphere_600x600_spp128.json")
GLASS = {"Glass": {"index_of_refraction": 1.5}}
METAL = {"Metal": {"albedo": [0.9, 0.9, 0.9], "fuzz": 0.05}}


def icosphere(c, r, subdivision):
    """the icosahedron's faces split in four `subdivision` times, every new vertex pushed out to the sphere: 20 * 4^subdivision faces"""
    verts, faces = icosahedron((0.0, 0.0, 0.0), 1.0)
    verts = [tuple(v) for v in verts]
    for _ in range(subdivision):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = [(verts[i][t] + verts[j][t]) / 2.0 for t in range(3)]
                ln = (m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) ** 0.5
                verts.append(tuple(x / ln for x in m))
                mid[key] = len(verts) - 1
            return mid[key]
        for i, j, k in faces:
            a, b, c2 = midpoint(i, j), midpoint(j, k), midpoint(k, i)
            out += [(i, a, c2), (j, b, a), (k, c2, b), (a, b, c2)]
        faces = out
    return [tuple(c[t] + r * v[t] for t in range(3)) for v in verts], faces


def room():
    white, red, green = _lam(0.73, 0.73, 0.73), _lam(0.65, 0.05, 0.05), _lam(0.12, 0.45, 0.15)
    return [
        _quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green),          # right
        _quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),              # left
        _quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white),            # floor
        _quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white),    # ceiling
        _quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white),          # back
        {"center": _pt(278, 480, 279), "radius": 60.0, "material": {"Light": {}}},
    ]


def make(subdivision=None):
    if subdivision is None:
        models = [_mesh(*icosphere((390.0, 110.0, 170.0), 105.0, 4), GLASS), _mesh(*icosphere((190.0, 125.0, 380.0), 120.0, 3), METAL)]
    else:
        models = [_mesh(*icosphere((278.0, 170.0, 300.0), 165.0, subdivision), METAL)]
    cfg = {"width": 600, "height": 600, "samples_per_pixel": 128, "max_depth": 50, "sky": None,
           "camera": {"look_from": _pt(278, 278, -800), "look_at": _pt(278, 278, 0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": 1.0},
           "objects": room() + models, "flat_bvh": True}
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivision", type=int, default=None, help="one Metal icosphere of this subdivision instead of the example's two")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(make(a.subdivision))
