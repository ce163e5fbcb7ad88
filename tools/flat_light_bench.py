#!/usr/bin/env python3
"""What area lights cost: kernel time by HIP events, median of 9 runs alternating in one process —
  1. the headline scene (scenes/cfg2_cover_1200x800_spp128.json): its code object is unchanged, its time is the control;
  2. the sphere-lamp Cornell room (scenes/cornell_spheres_600x600_spp128.json): the one existing workload that runs changed code (the lit
     QUADS megakernel, whose flat arm sits behind a wave-uniform false branch) — the frame must be the parent's in every bit;
  3. the panel room (scenes/cornell_panel_600x600_spp128.json): the same room lit by an emitting quad that is sampled.
GPU machine only.

    python tools/flat_light_bench.py [--reps 9] [--parent-lib DIR/librt_hip.so] [--out profiles/flat_lights_bench.json]

--parent-lib: librt_hip.so of the PARENT commit (built beside its own librt_host.so); frames 1 and 2 are then also rendered through it in
the same alternation, frame 2's bytes are compared, and its median is placed against the parent's own min - max band widened by 2 %.
Without it the file says so.  Reports ms, Msamples/s and segments per sample."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADLINE = "scenes/cfg2_cover_1200x800_spp128.json"
SPHERE_LAMP = "scenes/cornell_spheres_600x600_spp128.json"
PANEL = "scenes/cornell_panel_600x600_spp128.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_lights_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    parent = None
    if a.parent_lib:   # (an older library: the calls it lacks bind to stubs)
        os.environ["RT_SKIP_LAYOUT_CHECK"] = "1"
        parent = pkg.hip._bind(os.path.abspath(a.parent_lib), probes=False)
        del os.environ["RT_SKIP_LAYOUT_CHECK"]
    files = {"headline": HEADLINE, "sphere_lamp": SPHERE_LAMP, "panel": PANEL}
    scenes = {}

    def add(name, path, library=None):
        sc = pkg.host.Scene.load(path)
        gs = pkg.hip.HipScene(sc.ptr, 0, center1=sc.center1(), quads=sc.quads(), library=library)
        if library is None and sc.flat_emit() is not None:
            gs.set_flat_lights(sc.flat_emit())
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
    for name, path in files.items():
        add(name, path)
    if parent is not None:
        add("headline_parent_commit", HEADLINE, parent)
        add("sphere_lamp_parent_commit", SPHERE_LAMP, parent)
    order = (["headline_parent_commit", "sphere_lamp_parent_commit"] if parent is not None else []) + list(files)

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
                     "msamples_per_s": round(st["samples"] / med / 1e3, 1), "last_kernel": kern[name], "quads": max(gs.query("quads"), 0),
                     "n_lights": gs.query("n_lights"), "flat_lights": max(gs.query("flat_lights"), 0), "samples": st["samples"], "segments": st["segments"],
                     "segments_per_sample": round(st["segments"] / max(st["samples"], 1), 4)}
    out = {"reps": a.reps, "scenes": files, "parent_lib": bool(parent is not None), "runs": res}
    if parent is not None:
        torch.cuda.synchronize()
        same = bool(torch.equal(scenes["sphere_lamp"][2], scenes["sphere_lamp_parent_commit"][2]))
        p = res["sphere_lamp_parent_commit"]
        lo, hi = p["kernel_ms_min"] * 0.98, p["kernel_ms_max"] * 1.02
        out.update(sphere_lamp_frame_equals_parent=same,
                   sphere_lamp_over_parent_median=round(res["sphere_lamp"]["kernel_ms_median"] / p["kernel_ms_median"], 4),
                   sphere_lamp_parent_band_widened_2pc=[round(lo, 4), round(hi, 4)],
                   sphere_lamp_median_inside_band=bool(lo <= res["sphere_lamp"]["kernel_ms_median"] <= hi),
                   headline_over_parent_median=round(res["headline"]["kernel_ms_median"] / res["headline_parent_commit"]["kernel_ms_median"], 4))
    out["panel_over_sphere_lamp_median"] = round(res["panel"]["kernel_ms_median"] / res["sphere_lamp"]["kernel_ms_median"], 4)
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
