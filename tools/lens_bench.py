#!/usr/bin/env python3
"""What the thin lens costs: the example scene (scenes/cover_dof_1200x800_spp128.json, aperture 0.1, focus_dist
10) against the headline scene it is made from (cfg2, the pinhole).  GPU machine only.

    python tools/lens_bench.py [--reps 9] [--out profiles/lens_bench.json]

One-shot frames at 128 spp, and --denoise at 16 spp (rt_hip_refine_to_host_denoised: one pass, AOVs, filter), the two scenes
alternating rep by rep in one process; HIP events around each call (the kernel, or the host form's whole call); median, min, max."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = {"pinhole": "scenes/cfg2_cover_1200x800_spp128.json", "lens": "scenes/cover_dof_1200x800_spp128.json"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_bench.json"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    scenes = {}
    for name, path in SCENES.items():
        sc = pkg.host.Scene.load(path)
        cam, lens = (C.c_double * 11)(), (C.c_double * 2)()
        pkg.host.lib().rt_scene_camera(sc._h, cam)
        pkg.host.lib().rt_scene_lens(sc._h, lens)
        gs = pkg.hip.HipScene(sc.ptr, 0)
        if lens[0] != 0.0:
            d = pkg.host.camera_derive_lens(cam[0:3], cam[3:6], cam[6:9], cam[9], cam[10], lens[0], lens[1])
            gs.set_camera(d["origin"], d["lower_left_corner"], d["horizontal"], d["vertical"])
            gs.set_lens(d["u"], d["v"], d["lens_radius"])
        rgb = torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0")
        scenes[name] = (sc, gs, rgb)

    def one_shot(name):
        _, gs, rgb = scenes[name]
        gs.set_option("tile_order", 1)  # (bottom row first every frame: each frame the one-shot CLI frame's queue)
        gs.render(rgb.data_ptr(), 0, None, stream.cuda_stream)
        st = gs.wait()
        return st["kernel_ms"], st["segments"], gs.query("last_kernel")

    def denoised(name):
        _, gs, _ = scenes[name]
        gs.set_option("accum_reset", 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        gs.refine_to_host_denoised(16)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), None, gs.query("last_kernel")

    out = {"reps": a.reps, "scenes": SCENES, "runs": {}}
    for what, fn in (("one_shot_128spp_kernel_ms", one_shot), ("denoise_16spp_call_ms", denoised)):
        for name in SCENES:  # warm-up
            fn(name)
        v = {name: [] for name in SCENES}
        segs, kern = {}, {}
        for _ in range(a.reps):
            for name in SCENES:
                t, s, k = fn(name)
                v[name].append(t)
                if s is not None:
                    segs[name] = s
                kern[name] = k
        res = {name: {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "last_kernel": kern[name]}
               for name, x in v.items()}
        for name in segs:
            res[name]["segments"] = segs[name]
        res["lens_over_pinhole_median"] = round(res["lens"]["median"] / res["pinhole"]["median"], 4)
        out["runs"][what] = res
        print(what, json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
