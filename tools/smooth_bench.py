#!/usr/bin/env python3
"""What shading normals cost: kernel time by HIP events, median of 9 runs alternating in one process, this build beside
the PARENT commit's librt_hip.so —
  1. the headline scene (scenes/cfg2_cover_1200x800_spp128.json), parent and this build: the same code object, the ratio is reported;
  2. the Cornell mesh example (scenes/cornell_mesh_600x600_spp128.json) and the §22 icosphere scene (scenes/make_bvh_scene.py) WITHOUT
     normals, parent and this build: what every QUADS user pays for the branch;
  3. the icosphere scene WITH radial normals (scenes/make_smooth_scene.py) against the same build without: the feature's own cost.
The spread of each run (max - min of its repetitions) is written beside its median.  The icosphere frames are cut to --size and --spp
(the example's 600 x 600 at spp 128 takes seconds).  GPU machine only.

    python tools/smooth_bench.py --parent-lib DIR/librt_hip.so [--reps 9] [--size 300] [--spp 16] [--out profiles/smooth_normals_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
HEADLINE = "scenes/cfg2_cover_1200x800_spp128.json"
CORNELL_MESH = "scenes/cornell_mesh_600x600_spp128.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_normals_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft
    import make_smooth_scene

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    os.environ["RT_SKIP_LAYOUT_CHECK"] = "1"   # (an older library: the calls it lacks bind to stubs)
    parent = pkg.hip._bind(os.path.abspath(a.parent_lib), probes=False)
    del os.environ["RT_SKIP_LAYOUT_CHECK"]
    smooth = json.loads(make_smooth_scene.make())
    smooth.update(width=a.size, height=a.size, samples_per_pixel=a.spp)
    flat = json.loads(json.dumps(smooth))
    for o in flat["objects"]:
        o.get("mesh", {}).pop("normals", None)
    cfgs = {"headline": json.load(open(HEADLINE)), "cornell_mesh": json.load(open(CORNELL_MESH)), "icosphere": flat}
    scenes = {}

    def add(name, cfg, library, normals):
        sc = pkg.host.Scene.loads(json.dumps(cfg))
        quads = sc.quads()
        gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=sc.center1(), quads=quads, flat_bvh=sc.flat_bvh())
        if normals:
            gs.set_flat_normals(sc.flat_normals())
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
    for name, cfg in cfgs.items():
        add(name + "_parent", cfg, parent, False)
        add(name, cfg, None, False)
    add("icosphere_smooth", smooth, None, True)
    order = list(scenes)

    def one_shot(name):
        _, gs, rgb = scenes[name]
        gs.set_option("tile_order", 1)  # (bottom row first every frame: each frame the one-shot CLI frame's queue)
        gs.render(rgb.data_ptr(), 0, None, stream.cuda_stream)
        st = gs.wait()
        return st["kernel_ms"], st, gs.query("last_kernel")

    for name in order:  # warm-up
        one_shot(name)
    v, stats, kern = {name: [] for name in order}, {}, {}
    for _ in range(a.reps):
        for name in order:
            t, stats[name], kern[name] = one_shot(name)
            v[name].append(t)
    res = {}
    for name in order:
        st, gs = stats[name], scenes[name][1]
        med = statistics.median(v[name])
        res[name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(v[name]), 4), "kernel_ms_max": round(max(v[name]), 4),
                     "spread_ms": round(max(v[name]) - min(v[name]), 4), "msamples_per_s": round(st["samples"] / med / 1e3, 1), "last_kernel": kern[name],
                     "quads": max(gs.query("quads"), 0), "flat_normals": max(gs.query("flat_normals"), 0), "samples": st["samples"], "segments": st["segments"]}
    ratio = lambda x, y: round(res[x]["kernel_ms_median"] / res[y]["kernel_ms_median"], 4)
    out = {"reps": a.reps, "icosphere_frame": f"{a.size} x {a.size}, spp {a.spp}", "runs": res,
           "headline_over_parent": ratio("headline", "headline_parent"),
           "cornell_mesh_over_parent": ratio("cornell_mesh", "cornell_mesh_parent"),
           "icosphere_over_parent": ratio("icosphere", "icosphere_parent"),
           "icosphere_smooth_over_flat": ratio("icosphere_smooth", "icosphere")}
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
