#!/usr/bin/env python3
"""What triangles cost: four frames, kernel time by HIP events, median of 9 runs alternating in one process —
  1. the headline scene (scenes/cfg2_cover_1200x800_spp128.json): no flat primitive, the kernel it always ran;
  2. the Cornell example of §20 (scenes/cornell_spheres_600x600_spp128.json): 17 parallelograms, no triangle — quads_hit takes the loop of §20;
  3. the mesh example (scenes/cornell_mesh_600x600_spp128.json): 5 parallelograms and 34 triangles — the loop with the limit;
  4. the mesh example with every triangle turned into the parallelogram of the same Q, u, v: the same 39 entries through the loop of §20.
     Another picture (twice the area per entry), so its time is not frame 3's; it says what a 39-entry scan costs without the limit.
GPU machine only.

    python tools/tri_bench.py [--reps 9] [--parent-lib DIR/librt_hip.so] [--out profiles/tri_bench.json]

--parent-lib: librt_hip.so of the PARENT commit (built beside its own librt_host.so).  Frames 1, 2 and 4 — which the parent can render: it
ignores RtQuad.reserved — are then also rendered through it in the same alternation, and each is reported against it with the min - max of
both.  Reports Msamples/s and quad tests per segment (every segment tests every entry: their count)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADLINE = "scenes/cfg2_cover_1200x800_spp128.json"
CORNELL = "scenes/cornell_spheres_600x600_spp128.json"
MESH = "scenes/cornell_mesh_600x600_spp128.json"
PARENT_FRAMES = ("headline", "cornell", "mesh_as_parallelograms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_bench.json"))
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
    paths = {"headline": HEADLINE, "cornell": CORNELL, "mesh": MESH, "mesh_as_parallelograms": MESH}
    scenes = {}

    def add(name, frame, library):
        sc = pkg.host.Scene.load(paths[frame])
        quads = sc.quads()
        if frame == "mesh_as_parallelograms":
            for q in quads:
                q.reserved = pkg.abi.RT_QUAD_SHAPE_PARALLELOGRAM
        gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=sc.center1(), quads=quads)
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))

    order = []
    for frame in paths:
        if parent is not None and frame in PARENT_FRAMES:
            add(frame + "_parent_commit", frame, parent)
            order.append(frame + "_parent_commit")
        add(frame, frame, None)
        order.append(frame)

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
        seg, med = max(st["segments"], 1), statistics.median(v[name])
        quads = max(gs.query("quads"), 0)
        res[name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(v[name]), 4), "kernel_ms_max": round(max(v[name]), 4),
                     "msamples_per_s": round(st["samples"] / med / 1e3, 1), "last_kernel": kern[name], "quads": quads,
                     "triangles": max(gs.query("triangles"), 0), "quad_tests_per_segment": quads, "n_spheres": gs.query("n_spheres"),
                     "samples": st["samples"], "segments": st["segments"], "segments_per_sample": round(st["segments"] / max(st["samples"], 1), 4),
                     "ns_per_segment": round(med * 1e6 / seg, 3)}
    out = {"reps": a.reps, "scenes": paths, "parent_lib": bool(parent is not None), "runs": res}
    if parent is not None:
        out["this_over_parent_median"] = {f: round(res[f]["kernel_ms_median"] / res[f + "_parent_commit"]["kernel_ms_median"], 4) for f in PARENT_FRAMES}
        # the parent renders the same frames: the same paths, segment for segment
        out["same_segments_as_parent"] = {f: res[f]["segments"] == res[f + "_parent_commit"]["segments"] for f in PARENT_FRAMES}
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
