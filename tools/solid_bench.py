#!/usr/bin/env python3
"""What solid textures cost: the solid scene (scenes/cover_solid_1200x800_spp128.json: a checkered ground, a marble ball,
noise and turbulence spheres) against the headline scene it is made from (cfg2), and — to split the cost — the headline scene with one
hidden Noise sphere (radius 0.05 inside the first r = 0.2 sphere, which is opaque): the SOLID kernels on an otherwise equal workload,
i.e. the solid arm's presence in the shading alone, never taken.  GPU machine only.

    python tools/solid_bench.py [--reps 9] [--out profiles/solid_bench.json]

One-shot frames at 128 spp (kernel time by HIP events, exact tests and grid steps per segment), and --denoise at 16 spp
(rt_hip_refine_to_host_denoised: one pass, AOVs, filter), the three scenes alternating rep by rep in one process; median, min, max."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = {"static": "scenes/cfg2_cover_1200x800_spp128.json", "hidden_noise": "scenes/cfg2_cover_1200x800_spp128.json",
          "solid": "scenes/cover_solid_1200x800_spp128.json"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solid_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    scenes = {}
    for name, path in SCENES.items():
        cfg = json.load(open(path))
        if name == "hidden_noise":  # (inside the first small sphere: the grid's bounds, cells and `large` list stay the static scene's)
            c = cfg["objects"][1]["center"]
            assert cfg["objects"][1]["radius"] == 0.2 and "Glass" not in cfg["objects"][1]["material"]
            cfg["objects"].append({"center": dict(c), "radius": 0.05, "material": {"Noise": {"albedo": [0.5, 0.5, 0.5], "scale": 4.0}}})
        sc = pkg.host.Scene.loads(json.dumps(cfg))
        gs = pkg.hip.HipScene(sc.ptr, 0, center1=sc.center1())
        rgb = torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0")
        scenes[name] = (sc, gs, rgb)

    def one_shot(name):
        _, gs, rgb = scenes[name]
        gs.set_option("tile_order", 1)  # (bottom row first every frame: each frame the one-shot CLI frame's queue)
        gs.render(rgb.data_ptr(), 0, None, stream.cuda_stream)
        st = gs.wait()
        return st["kernel_ms"], st, gs.query("last_kernel")

    def denoised(name):
        _, gs, _ = scenes[name]
        gs.set_option("accum_reset", 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        gs.refine_to_host_denoised(16)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), None, gs.query("last_kernel")

    out = {"reps": a.reps, "scenes": SCENES, "tables": {}, "runs": {}}
    for name, (_, gs, _) in scenes.items():
        out["tables"][name] = {k: gs.query(k) for k in ("n_spheres", "solids", "grid_cells", "grid_items", "grid_large", "lds_tables")}
    for what, fn in (("one_shot_128spp_kernel_ms", one_shot), ("denoise_16spp_call_ms", denoised)):
        for name in SCENES:  # warm-up
            fn(name)
        v = {name: [] for name in SCENES}
        stats, kern = {}, {}
        for _ in range(a.reps):
            for name in SCENES:
                t, st, k = fn(name)
                v[name].append(t)
                if st is not None:
                    stats[name] = st
                kern[name] = k
        res = {name: {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "last_kernel": kern[name]}
               for name, x in v.items()}
        for name, st in stats.items():
            seg = max(st["segments"], 1)
            res[name]["segments"] = st["segments"]
            res[name]["segments_per_sample"] = round(st["segments"] / max(st["samples"], 1), 4)
            res[name]["exact_tests_per_segment"] = round(st["exact_tests"] / seg, 4)
            res[name]["grid_steps_per_segment"] = round(st["grid_steps"] / seg, 4)
            res[name]["lds_tables"] = scenes[name][1].query("lds_tables")
        for name in ("hidden_noise", "solid"):
            res[f"{name}_over_static_median"] = round(res[name]["median"] / res["static"]["median"], 4)
        out["runs"][what] = res
        print(what, json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
