#!/usr/bin/env python3
"""What images on flat primitives cost: kernel time by HIP events, median of 9 runs alternating in one process —
  1. the headline scene (scenes/cfg2_cover_1200x800_spp128.json): its code object is unchanged, its time is the control;
  2. the existing QUADS workloads, which now run changed code with the bit unset (the image arm sits behind a wave-uniform false branch):
     scenes/cornell_spheres_600x600_spp128.json (key 516), scenes/cornell_mesh_600x600_spp128.json and the icosphere room with its
     structure (scenes/make_bvh_scene.py) — each frame must be the parent's in every bit;
  3. the example scenes/cornell_image_600x600_spp128.json against the same room without images (scenes/make_cornell_image_scene.py --plain).
GPU machine only.

    python tools/flat_image_bench.py [--reps 9] [--parent-lib DIR/librt_hip.so] [--out profiles/flat_images_bench.json]

--parent-lib: librt_hip.so of the PARENT commit (built beside its own librt_host.so); the frames of 1 and 2 are then also rendered through
it in the same alternation, their bytes are compared, and each median is placed against the parent's own min - max band widened by 2 %.
Without it the file says so.  Reports ms, Msamples/s and segments per sample."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
HEADLINE = "scenes/cfg2_cover_1200x800_spp128.json"
EXISTING = {"cornell_spheres": "scenes/cornell_spheres_600x600_spp128.json", "cornell_mesh": "scenes/cornell_mesh_600x600_spp128.json"}
IMAGE = "scenes/cornell_image_600x600_spp128.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_images_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft
    import make_bvh_scene
    import make_cornell_image_scene

    os.chdir(ROOT)
    pkg = graft.load_package()
    stream = torch.cuda.current_stream()
    parent = None
    if a.parent_lib:   # (an older library: the calls it lacks bind to stubs)
        os.environ["RT_SKIP_LAYOUT_CHECK"] = "1"
        parent = pkg.hip._bind(os.path.abspath(a.parent_lib), probes=False)
        del os.environ["RT_SKIP_LAYOUT_CHECK"]
    tmp = tempfile.mkdtemp(prefix="flat_image_bench_")
    generated = {"icosphere_bvh": make_bvh_scene.make(), "image_room_plain": make_cornell_image_scene.make(plain=True)}
    for name, text in generated.items():
        with open(os.path.join(tmp, name + ".json"), "w") as f:
            f.write(text)
    files = {"headline": HEADLINE, **EXISTING, "icosphere_bvh": os.path.join(tmp, "icosphere_bvh.json"),
             "image_room_plain": os.path.join(tmp, "image_room_plain.json"), "image_room": IMAGE}
    compared = ["headline", *EXISTING, "icosphere_bvh"]     # what the parent renders too
    scenes = {}

    def add(name, path, library=None):
        sc = pkg.host.Scene.load(path)
        gs = pkg.hip.HipScene(sc.ptr, 0, center1=sc.center1(), quads=sc.quads(), flat_bvh=sc.flat_bvh(), library=library)
        if sc.flat_normals() is not None:
            gs.set_flat_normals(sc.flat_normals())
        if library is None and sc.flat_images() is not None:
            gs.set_flat_images(sc.flat_images())
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
    for name, path in files.items():
        add(name, path)
    if parent is not None:
        for name in compared:
            add(name + "_parent_commit", files[name], parent)
    order = ([n + "_parent_commit" for n in compared] if parent is not None else []) + list(files)

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
                     "flat_images": max(gs.query("flat_images"), 0), "samples": st["samples"], "segments": st["segments"],
                     "segments_per_sample": round(st["segments"] / max(st["samples"], 1), 4)}
    out = {"reps": a.reps, "scenes": {k: (v if not v.startswith(tmp) else "generated: " + k) for k, v in files.items()}, "parent_lib": bool(parent is not None),
           "runs": res}
    if parent is not None:
        torch.cuda.synchronize()
        against = {}
        for name in compared:
            p = res[name + "_parent_commit"]
            lo, hi = p["kernel_ms_min"] * 0.98, p["kernel_ms_max"] * 1.02
            against[name] = {"frame_equals_parent": bool(torch.equal(scenes[name][2], scenes[name + "_parent_commit"][2])),
                             "over_parent_median": round(res[name]["kernel_ms_median"] / p["kernel_ms_median"], 4),
                             "parent_band_widened_2pc": [round(lo, 4), round(hi, 4)],
                             "median_inside_band": bool(lo <= res[name]["kernel_ms_median"] <= hi)}
        out["against_parent"] = against
    out["image_room_over_plain_median"] = round(res["image_room"]["kernel_ms_median"] / res["image_room_plain"]["kernel_ms_median"], 4)
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
