#!/usr/bin/env python3
"""What building the flat-primitive BVH anew costs on the host and on the device.  GPU machine only.

    python tools/analysis/flat_device_build_time.py [--reps 24] [--out profiles/flat_device_build_time.json]

The two worlds of tools/analysis/flat_update_time.py — the example icosphere scene (6 400 faces and five walls) and a heightfield of 2^18
triangles — and four ways to get the next frame's geometry into the scene, alternated in ONE process, a host clock around each blocking
call (the method of §24):
    refit                 rt_hip_scene_update_flats from host memory
    rebuild_host          ... with RT_UPDATE_FLATS_REBUILD, option "flat_build" 0: the host's build_flat_bvh
    rebuild_device        ... option "flat_build" 1, geometry in host memory
    rebuild_device_tensor ... option "flat_build" 1, RT_UPDATE_FLATS_DEVICE from a tensor on the scene's device
Median, quartiles, minimum and maximum over --reps repetitions after two warm-up rounds; every rebuilt table is compared with the host
build's once, byte for byte.  Then what a caller buys: the frame's kernel ms after a scramble (every entry moved to another entry's
place) applied by refit, against the same geometry after a device rebuild."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_device_build_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    abi, hip, host = pkg.abi, pkg.hip, pkg.host
    assert torch.cuda.is_available(), "needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream

    def quv_of(flats):
        return np.frombuffer(flats, np.uint8).reshape(len(flats), C.sizeof(abi.RtQuad))[:, :72].copy().view(np.float64)

    def with_quv(flats, quv):
        out = (abi.RtQuad * len(flats))()
        C.memmove(out, flats, C.sizeof(out))
        np.frombuffer(out, np.uint8).reshape(len(flats), C.sizeof(abi.RtQuad))[:, :72] = np.ascontiguousarray(quv).view(np.uint8).reshape(len(flats), 72)
        return out

    # ---- the worlds: (scene pointer, flats, phase -> quv)
    def icosphere_world():
        sys.path.insert(0, os.path.join(ROOT, "scenes"))
        spec = importlib.util.spec_from_file_location("make_bvh_scene", os.path.join(ROOT, "scenes", "make_bvh_scene.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sc = host.Scene.loads(mod.make())
        sc.c.width, sc.c.height, sc.c.samples_per_pixel, sc.c.max_depth = 300, 300, 16, 16
        flats = sc.quads()
        base = quv_of(flats)

        def at(phase):   # the two models wobble sideways, every triangle by its own height (the five walls stay)
            q = base.copy()
            q[5:, 0] += 12.0 * np.sin(phase + q[5:, 1] / 30.0)
            q[5:, 2] += 8.0 * np.cos(0.7 * phase + q[5:, 1] / 45.0)
            return q
        return sc, sc.ptr, flats, at

    def heightfield_world():
        nx, nz = 512, 256                                    # 2 * 512 * 256 = 2^18 triangles
        xs, zs = np.linspace(-5, 5, nx + 1), np.linspace(-5, 5, nz + 1)
        X, Z = np.meshgrid(xs, zs, indexing="ij")
        spheres = (abi.RtSphere * 1)()
        spheres[0].center[:] = [0.5, 1.6, 0.3]
        spheres[0].radius = 0.6
        spheres[0].albedo[:] = [0.6, 0.5, 0.7]
        sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=480, height=320, samples_per_pixel=8, max_depth=8, sky_mode=abi.RT_SKY_GRADIENT, spheres=spheres,
                         n_spheres=1, seed=4711)
        sc.cam_origin[:] = [0.0, 9.0, 0.5]
        sc.cam_lower_left[:] = [-5.0, 0.0, -5.0]; sc.cam_horizontal[:] = [10.0, 0.0, 0.0]; sc.cam_vertical[:] = [0.0, 0.0, 10.0]

        def at(phase):
            Y = 0.3 + 0.25 * np.sin(1.7 * X + phase) * np.cos(1.3 * Z - 0.5 * phase)
            P = np.stack([X, Y, Z], axis=2)
            a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
            t0 = np.concatenate([a, c - a, b - a], axis=2)
            t1 = np.concatenate([a, d - a, c - a], axis=2)
            return np.ascontiguousarray(np.stack([t0, t1], axis=2).reshape(-1, 9))
        base = at(0.0)
        flats = (abi.RtQuad * len(base))()
        rec = np.frombuffer(flats, np.uint8).reshape(len(base), C.sizeof(abi.RtQuad))
        rec[:, :72] = base.view(np.uint8).reshape(len(base), 72)
        tmpl = abi.RtQuad(fuzz_or_ior=1.5, kind=abi.RT_MAT_LAMBERTIAN, reserved=abi.RT_QUAD_SHAPE_TRIANGLE)
        tmpl.albedo[:] = [0.7, 0.6, 0.5]
        rec[:, 72:] = np.frombuffer(bytes(tmpl), np.uint8)[72:]
        return (sc, spheres), C.pointer(sc), flats, at

    def kernel_ms(gs, w, h, reps=5):
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        out = []
        for _ in range(reps + 1):
            gs.render(rgb.data_ptr(), 0, None, stream)
            out.append(gs.wait()["kernel_ms"])
        return round(statistics.median(out[1:]), 4)

    result = {"reps": a.reps, "worlds": {}}
    for name, make in (("icosphere_6400", icosphere_world), ("heightfield_2e18", heightfield_world)):
        keep, ptr, flats, at = make()
        phases = [at(0.4 * k) for k in range(1, 5)]
        d_phases = [torch.from_numpy(p).to("cuda:0") for p in phases]
        gs = hip.HipScene(ptr, 0, quads=flats, flat_bvh=True)
        w, h = gs.width, gs.height
        times = {"refit": [], "rebuild_host": [], "rebuild_device": [], "rebuild_device_tensor": []}
        tables = {}
        for rep in range(a.reps + 2):
            k = rep % len(phases)
            for variant in times:
                gs.set_option("flat_build", 1 if "device" in variant else 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if variant == "refit":
                    gs.update_flats(phases[k])
                elif variant == "rebuild_device_tensor":
                    gs.update_flats(d_phases[k], rebuild=True)
                else:
                    gs.update_flats(phases[k], rebuild=True)
                ms = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    times[variant].append(ms)
                if rep == 0 and variant != "refit":
                    tables[variant] = (gs.table("flat_bvh"), gs.table("flat_bvh_order"))
        assert tables["rebuild_device"] == tables["rebuild_host"] and tables["rebuild_device_tensor"] == tables["rebuild_host"]
        assert gs.query("flat_device_builds") == 2 * (a.reps + 2)
        entry = {"flat_primitives": len(flats), "nodes": gs.query("flat_bvh"), "update_ms": {v: _spread(ms) for v, ms in times.items()}}
        # what a caller buys: a scramble applied by refit against the same geometry after a device rebuild
        rng = np.random.default_rng(900)
        base = at(0.0)
        scrambled = base.copy()
        first = 5 if name.startswith("icosphere") else 0          # (the icosphere scene's five walls stay)
        perm = first + rng.permutation(len(base) - first)
        scrambled[first:, :3] = base[perm, :3]
        quality = {}
        gs.set_option("flat_build", 1)
        gs.update_flats(base, rebuild=True)
        quality["built"] = kernel_ms(gs, w, h)
        gs.update_flats(scrambled)
        assert gs.query("flat_refits") == 1
        quality["scrambled_refit"] = kernel_ms(gs, w, h)
        gs.update_flats(scrambled, rebuild=True)
        assert gs.query("flat_refits") == 0
        quality["scrambled_device_rebuild"] = kernel_ms(gs, w, h)
        entry["frame"] = {"width": w, "height": h, "kernel_ms": quality}
        result["worlds"][name] = entry
        gs.close()
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
