#!/usr/bin/env python3
"""What motion of the flat primitives within the frame costs: kernel time by HIP events, median of 9 runs alternating in
one process, this build beside the PARENT commit's librt_hip.so —
  1. the headline scene (scenes/cfg2_cover_1200x800_spp128.json), parent and this build: the same code object, the ratio is reported;
  2. the Cornell mesh example (scenes/cornell_mesh_600x600_spp128.json) with one small moving sphere added — still flat primitives under
     the QUADS ∧ MOTION kernels, a scene both libraries render — parent and this build: what the new wave-uniform branch costs a scene
     that had the key already, beside the parent's own min - max spread;
  3. the example (scenes/make_flat_motion_scene.py) still;
  4. the example moving: the feature's own cost, with segments per frame; its box and entry tests per segment come from the CPU build of the
     lane code on a 48 x 48 cut (the device has no such counters).
The frames of 2 - 4 are cut to --size and --spp.  GPU machine only.

    python tools/flat_motion_bench.py --parent-lib DIR/librt_hip.so [--reps 9] [--size 300] [--spp 16] [--out profiles/flat_motion_bench.json]"""
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


def cpu_cut_counts(pkg, make_flat_motion_scene):
    """frame 4's work per segment, which the device has no counters for: the CPU build of the lane code (tests/flat_motion_sim.py, the
    walk's counters compiled in) on a 48 x 48, spp 4, depth 8 cut of the example, still against moving"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import flat_motion_sim
    sim, res = flat_motion_sim.load(pkg.abi), {}
    for name, still in (("still", True), ("moving", False)):
        cfg = json.loads(make_flat_motion_scene.make(still=still))
        cfg.update(width=48, height=48, samples_per_pixel=4, max_depth=8)
        sc = pkg.host.Scene.loads(json.dumps(cfg))
        rc, _, _, segs, _, cnt = sim.render(sc.c, sc.quads(), sc.flat_motion(), sc.flat_normals(), None, flat_bvh=True)
        assert rc == 0
        res[name] = {"segments": segs, "box_tests_per_segment": round(cnt["box_tests"] / segs, 2), "entry_tests_per_segment": round(cnt["entry_tests"] / segs, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_motion_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft
    import make_flat_motion_scene

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    os.environ["RT_SKIP_LAYOUT_CHECK"] = "1"   # (an older library: the calls it lacks bind to stubs)
    parent = pkg.hip._bind(os.path.abspath(a.parent_lib), probes=False)
    del os.environ["RT_SKIP_LAYOUT_CHECK"]

    def cut(cfg):
        cfg.update(width=a.size, height=a.size, samples_per_pixel=a.spp)
        return cfg
    spheres_move = cut(json.load(open(CORNELL_MESH)))
    spheres_move["objects"].append({"center": {"x": 150.0, "y": 330.0, "z": 200.0}, "center1": {"x": 190.0, "y": 300.0, "z": 200.0}, "radius": 40.0,
                                    "material": {"Lambertian": {"albedo": [0.3, 0.3, 0.8]}}})
    cfgs = {"headline": (json.load(open(HEADLINE)), True), "spheres_move": (spheres_move, True),
            "example_still": (cut(json.loads(make_flat_motion_scene.make(still=True))), False),
            "example_moving": (cut(json.loads(make_flat_motion_scene.make())), False)}
    scenes = {}

    def add(name, cfg, library):
        sc = pkg.host.Scene.loads(json.dumps(cfg))
        quads = sc.quads()
        gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=sc.center1(), quads=quads, flat_bvh=sc.flat_bvh())
        if library is None and sc.flat_normals() is not None:
            gs.set_flat_normals(sc.flat_normals())
        if library is None and sc.flat_motion() is not None:
            gs.set_flat_motion(sc.flat_motion())
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
    for name, (cfg, both) in cfgs.items():
        if both:
            add(name + "_parent", cfg, parent)
        add(name, cfg, None)
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
                     "quads": max(gs.query("quads"), 0), "flat_motion": max(gs.query("flat_motion"), 0) if not name.endswith("_parent") else 0,
                     "samples": st["samples"], "segments": st["segments"]}
    ratio = lambda x, y: round(res[x]["kernel_ms_median"] / res[y]["kernel_ms_median"], 4)
    p = res["spheres_move_parent"]
    out = {"reps": a.reps, "cut_frames": f"{a.size} x {a.size}, spp {a.spp}", "runs": res,
           "headline_over_parent": ratio("headline", "headline_parent"),
           "spheres_move_over_parent": ratio("spheres_move", "spheres_move_parent"),
           "spheres_move_parent_max_over_min": round(p["kernel_ms_max"] / p["kernel_ms_min"], 4),
           "example_moving_over_still": ratio("example_moving", "example_still")}
    out["example_cpu_cut_48x48_spp4"] = cpu_cut_counts(pkg, make_flat_motion_scene)
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
