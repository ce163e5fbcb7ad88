#!/usr/bin/env python3
"""What the structure over the flat primitives costs and buys: kernel time by HIP events, median of 9 runs alternating in
one process, min - max, Msamples/s and segments per sample for each frame —
  headline                      scenes/cfg2_cover_1200x800_spp128.json: parent and this build (no flat primitive)
  cornell (17 entries, §20)     parent scan, this scan, this structure
  mesh (39 entries, §21)        parent scan, this scan, this structure
  ico3_1024                     an icosphere at subdivision 3 cut to 1 019 faces + the room's 5 walls = the old cap: this scan, this structure
  example (6 405 entries)       the example scenes/make_bvh_scene.py writes: structure only
  ico6 (81 925 entries)         an icosphere at subdivision 6 in the room: structure only; the host build time (scene creation) is reported
GPU machine only.  The frames past the headline are rendered at --size (default 300 x 300) and --spp (default 32) so that the whole run
fits a few minutes; the headline at its own size.

    python tools/flat_bvh_bench.py [--reps 9] [--parent-lib DIR/librt_hip.so] [--out profiles/flat_bvh_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
HEADLINE = "scenes/cfg2_cover_1200x800_spp128.json"
CORNELL = "scenes/cornell_spheres_600x600_spp128.json"
MESH = "scenes/cornell_mesh_600x600_spp128.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-ico6", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_bvh_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft
    import make_bvh_scene

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    parent = None
    if a.parent_lib:   # (an older library: the calls it lacks bind to stubs)
        os.environ["RT_SKIP_LAYOUT_CHECK"] = "1"
        parent = pkg.hip._bind(os.path.abspath(a.parent_lib), probes=False)
        del os.environ["RT_SKIP_LAYOUT_CHECK"]
    tmp = tempfile.mkdtemp(prefix="flat_bvh_bench_")
    paths = {"headline": HEADLINE, "cornell": CORNELL, "mesh": MESH, "example": os.path.join(tmp, "example.json")}
    with open(paths["example"], "w") as f:
        f.write(make_bvh_scene.make())
    for name, sub in (("ico3_1024", 3),) + (() if a.skip_ico6 else (("ico6", 6),)):
        cfg = json.loads(make_bvh_scene.make(sub))
        if name == "ico3_1024":
            cfg["objects"][-1]["mesh"]["faces"] = cfg["objects"][-1]["mesh"]["faces"][:1019]
        paths[name] = os.path.join(tmp, name + ".json")
        with open(paths[name], "w") as f:
            json.dump(cfg, f)
    scenes, order, build_ms = {}, [], {}

    def add(name, frame, library, bvh):
        sc = pkg.host.Scene.load(paths[frame])
        if frame != "headline":
            sc.c.width = sc.c.height = a.size
            sc.c.samples_per_pixel = a.spp
        t0 = time.perf_counter()
        gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=sc.center1(), quads=sc.quads(), flat_bvh=bvh)
        build_ms[name] = round((time.perf_counter() - t0) * 1e3, 2)
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
        order.append(name)

    for frame in paths:
        small = frame in ("cornell", "mesh")
        if parent is not None and (small or frame == "headline"):
            add(frame + "_parent_scan", frame, parent, False)
        if frame == "headline":
            add("headline", frame, None, False)
            continue
        if small or frame == "ico3_1024":
            add(frame + "_scan", frame, None, False)
        add(frame + "_bvh", frame, None, True)

    def one_shot(name):
        _, gs, rgb = scenes[name]
        gs.set_option("tile_order", 1)  # (bottom row first every frame: each frame the one-shot CLI frame's queue)
        gs.render(rgb.data_ptr(), 0, None, stream.cuda_stream)
        st = gs.wait()
        return st["kernel_ms"], st, gs.query("last_kernel")

    frames = {}
    for name in order:  # warm-up; the routes of one frame render the same picture
        one_shot(name)
        frames[name] = scenes[name][2].cpu().numpy().tobytes()
    v, stats, kern = {name: [] for name in order}, {}, {}
    for _ in range(a.reps):
        for name in order:
            t, stats[name], kern[name] = one_shot(name)
            v[name].append(t)
    res = {}
    for name in order:
        st, gs = stats[name], scenes[name][1]
        seg, med = max(st["segments"], 1), statistics.median(v[name])
        res[name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(v[name]), 4), "kernel_ms_max": round(max(v[name]), 4),
                     "msamples_per_s": round(st["samples"] / med / 1e3, 1), "last_kernel": kern[name], "quads": max(gs.query("quads"), 0),
                     "flat_bvh_nodes": max(gs.query("flat_bvh"), 0), "samples": st["samples"], "segments": st["segments"],
                     "segments_per_sample": round(st["segments"] / max(st["samples"], 1), 4), "ns_per_segment": round(med * 1e6 / seg, 3),
                     "scene_create_ms": build_ms[name]}
    out = {"reps": a.reps, "size": a.size, "spp": a.spp, "parent_lib": bool(parent is not None), "runs": res}
    # the AOV and surface kernels on §20's room (rt_aov_quads, rt_surface_quads: their register figures grew): torch events around each call
    side = {}
    names = [n for n in order if n.startswith("cornell_")]
    bufs = {n: (torch.zeros((scenes[n][0].c.height, scenes[n][0].c.width, 8), dtype=torch.float32, device="cuda:0"),
                torch.zeros((scenes[n][0].c.height, scenes[n][0].c.width, 2), dtype=torch.float64, device="cuda:0")) for n in names}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    tv = {n: {"aovs": [], "surface": []} for n in names}
    for rep in range(a.reps + 1):
        for n in names:
            gs, (aov, surf) = scenes[n][1], bufs[n]
            ta = timed(lambda: gs.render_aovs(a.spp, aov.data_ptr(), None, stream.cuda_stream))
            ts = timed(lambda: gs.render_surface(surf.data_ptr(), None, stream.cuda_stream))
            if rep:   # (the first round warms up)
                tv[n]["aovs"].append(ta); tv[n]["surface"].append(ts)
    for n in names:
        side[n] = {k: {"ms_median": round(statistics.median(x), 4), "ms_min": round(min(x), 4), "ms_max": round(max(x), 4)} for k, x in tv[n].items()}
    out["cornell_aovs_and_surface"] = side
    same = {}
    for frame in ("cornell", "mesh", "ico3_1024"):
        names = [n for n in order if n.startswith(frame + "_")]
        same[frame] = all(frames[n] == frames[names[0]] for n in names)
    out["routes_render_the_same_bytes"] = same
    if parent is not None:   # the bar: this build's scan median <= the parent's own maximum x 1.01
        out["scan_bar"] = {f: {"this_scan_median": res[f + "_scan"]["kernel_ms_median"], "parent_max_x_1.01": round(res[f + "_parent_scan"]["kernel_ms_max"] * 1.01, 4),
                               "this_over_parent_median": round(res[f + "_scan"]["kernel_ms_median"] / res[f + "_parent_scan"]["kernel_ms_median"], 4),
                               "met": res[f + "_scan"]["kernel_ms_median"] <= res[f + "_parent_scan"]["kernel_ms_max"] * 1.01} for f in ("cornell", "mesh")}
        out["headline_this_over_parent_median"] = round(res["headline"]["kernel_ms_median"] / res["headline_parent_scan"]["kernel_ms_median"], 4)
    out["bvh_over_scan_median"] = {f: round(res[f + "_bvh"]["kernel_ms_median"] / res[f + "_scan"]["kernel_ms_median"], 4) for f in ("cornell", "mesh", "ico3_1024")}
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        head = ",\n ".join(json.dumps(k) + ": " + json.dumps(x) for k, x in out.items() if k != "runs")   # (one run per line)
        f.write("{" + head + ',\n "runs": {\n  ' + ",\n  ".join(json.dumps(k) + ": " + json.dumps(x) for k, x in res.items()) + "\n }}\n")
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
