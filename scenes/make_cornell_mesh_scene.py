"""scenes/cornell_mesh_600x600_spp128.json: the room of scenes/make_cornell_scene.py with meshes in place of the two boxes —
a Lambertian pyramid (6 triangles), a Glass octahedron (8) and a Metal icosahedron (20), each a {"mesh": {"vertices", "faces"}} object;
34 triangles beside the five wall quads.  Every face is wound counter-clockwise seen from outside, so N = cross(u, v) points outward: the
glass gem's front_face is right (a Lambertian or Metal triangle does not read it).  The lamp is the sphere Light of the room.

    python scenes/make_cornell_mesh_scene.py        # rewrites the file (deterministic)"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cornell_mesh_600x600_spp128.json")


def _pt(x, y, z):
    return {"x": float(x), "y": float(y), "z": float(z)}


def _quad(q, u, v, mat):
    return {"q": _pt(*q), "u": _pt(*u), "v": _pt(*v), "material": mat}


def _lam(r, g, b):
    return {"Lambertian": {"albedo": [r, g, b]}}


def _outward(vertices, faces):
    """each face (i, j, k) with cross(b - a, c - a) pointing away from the mesh's centre (convex meshes): j and k change places otherwise"""
    n = float(len(vertices))
    centre = [sum(v[c] for v in vertices) / n for c in range(3)]
    out = []
    for i, j, k in faces:
        a, b, c = vertices[i], vertices[j], vertices[k]
        u, v = [b[t] - a[t] for t in range(3)], [c[t] - a[t] for t in range(3)]
        nrm = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        mid = [(a[t] + b[t] + c[t]) / 3.0 - centre[t] for t in range(3)]
        out.append([i, j, k] if sum(nrm[t] * mid[t] for t in range(3)) > 0.0 else [i, k, j])
    return out


def _mesh(vertices, faces, mat):
    vertices = [[round(float(x), 3) for x in v] for v in vertices]
    return {"mesh": {"vertices": vertices, "faces": _outward(vertices, faces)}, "material": mat}


def pyramid(x0, z0, side, height):
    v = [(x0, 0.0, z0), (x0 + side, 0.0, z0), (x0 + side, 0.0, z0 + side), (x0, 0.0, z0 + side), (x0 + side / 2.0, height, z0 + side / 2.0)]
    return v, [(0, 1, 2), (0, 2, 3), (0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)]


def octahedron(c, r):
    v = [(c[0] + r, c[1], c[2]), (c[0] - r, c[1], c[2]), (c[0], c[1] + r, c[2]), (c[0], c[1] - r, c[2]), (c[0], c[1], c[2] + r), (c[0], c[1], c[2] - r)]
    return v, [(x, y, z) for x in (0, 1) for y in (2, 3) for z in (4, 5)]


def icosahedron(c, r):
    phi = (1.0 + 5.0 ** 0.5) / 2.0
    s = r / (1.0 + phi * phi) ** 0.5
    raw = [(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi), (phi, 0, -1), (phi, 0, 1),
           (-phi, 0, -1), (-phi, 0, 1)]
    v = [tuple(c[t] + s * p[t] for t in range(3)) for p in raw]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return v, f


def objects():
    white, red, green = _lam(0.73, 0.73, 0.73), _lam(0.65, 0.05, 0.05), _lam(0.12, 0.45, 0.15)
    return [
        _quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green),          # right
        _quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),              # left
        _quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white),            # floor
        _quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white),    # ceiling
        _quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white),          # back
        {"center": _pt(278, 480, 279), "radius": 60.0, "material": {"Light": {}}},
        _mesh(*pyramid(90.0, 70.0, 170.0, 190.0), _lam(0.8, 0.6, 0.2)),
        _mesh(*octahedron((410.0, 100.0, 140.0), 95.0), {"Glass": {"index_of_refraction": 1.5}}),
        _mesh(*icosahedron((300.0, 115.0, 400.0), 110.0), {"Metal": {"albedo": [0.9, 0.9, 0.9], "fuzz": 0.05}}),
    ]


def make():
    cfg = {"width": 600, "height": 600, "samples_per_pixel": 128, "max_depth": 50, "sky": None,
           "camera": {"look_from": _pt(278, 278, -800), "look_at": _pt(278, 278, 0), "vup": _pt(0, 1, 0), "vfov": 40.0, "aspect": 1.0},
           "objects": objects()}
    return json.dumps(cfg, separators=(",", ":"))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(make())
