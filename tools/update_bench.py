#!/usr/bin/env python3
"""What moving the spheres of a resident scene costs, on the GPU.

    python tools/update_bench.py [--reps 20] [--out profiles/update_bench.json]

For lattice worlds of 488, 10 004 and 202 504 spheres: the wall time of rt_hip_scene_update_spheres, and next to it what the same
move costs without it: rt_hip_scene_destroy + rt_hip_scene_create_moving at the new centres.  Every figure is the median of --reps
repetitions after 3 warm-up repetitions, with min and max; the centres alternate between two sets, so every repetition rebuilds
another grid.  The split of an update into its stages comes from rt_hip_setup_profile (host plan, upload, count kernels + the
readback that waits for them, table kernels, configuration), the medians over the same repetitions.  Last: frames per second of
`raytracer scenes/cover_motion_1200x800_spp128.json --frames 32 --shutter 0.5` (RT_STATS=1), best of 3 runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime in the process, torch's)
    import __graft_entry__ as graft
    import procedural
    from update_worlds import centres_of, set_centres
    pkg = graft.load_package()
    host, hip = pkg.host, pkg.hip
    os.chdir(ROOT)
    result = {"reps": a.reps, "worlds": {}}
    for half in (11, 50, 225):
        cfg = procedural.make_config(width=64, height=48, spp=2, max_depth=8, half=half)
        n = len(cfg["objects"])
        sc = host.Scene.loads(json.dumps(cfg))
        base = centres_of(cfg)
        rng = np.random.default_rng(half)
        small = np.array([abs(o["radius"]) < 0.5 for o in cfg["objects"]])
        sets = []
        for _ in range(2):
            c = base.copy()
            c[small] += rng.uniform(-0.2, 0.2, (int(small.sum()), 3)) * np.array([1.0, 0.0, 1.0])
            sets.append(c)
        gs = hip.HipScene(sc.ptr, 0)
        upd, stages = [], {}
        for i in range(a.reps + 3):
            c = sets[i & 1]
            t0 = time.perf_counter()
            gs.update_spheres(c)
            ms = (time.perf_counter() - t0) * 1e3
            if i >= 3:
                upd.append(ms)
                for k, v in hip.setup_profile().items():
                    stages.setdefault(k, []).append(v)
        tables = {q: gs.query(q) for q in ("grid_cells", "grid_items", "grid_wide", "grid_large", "table_bytes")}
        gs.close()
        # the parent's way: destroy the scene, create it again at the new centres (the RtScene already holds them: patching the
        # caller's own sphere array is not counted)
        rec = []
        gs = hip.HipScene(sc.ptr, 0)
        for i in range(a.reps + 3):
            set_centres(pkg.abi, sc, sets[i & 1])
            t0 = time.perf_counter()
            gs.close()
            gs = hip.HipScene(sc.ptr, 0)
            ms = (time.perf_counter() - t0) * 1e3
            if i >= 3:
                rec.append(ms)
        gs.close()
        u, r = summary(upd), summary(rec)
        faster = u["max_ms"] < r["min_ms"]   # beyond the run-to-run spread of both: the slowest update against the fastest re-creation
        result["worlds"][str(n)] = {"spheres": n, "update_spheres": u, "destroy_and_create": r, "update_stages_median_ms": {k: round(statistics.median(v), 4) for k, v in stages.items()},
                                   "speedup_of_medians": round(r["median_ms"] / u["median_ms"], 3), "update_faster_beyond_spread": faster, **tables}
        print(json.dumps({n: result["worlds"][str(n)]}), flush=True)
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    fps = []
    with tempfile.TemporaryDirectory() as td:
        for _ in range(3):
            r = subprocess.run([exe, "scenes/cover_motion_1200x800_spp128.json", os.path.join(td, "f"), "--frames", "32", "--shutter", "0.5"],
                               capture_output=True, text=True, timeout=600, env=dict(os.environ, RT_STATS="1"))
            if r.returncode != 0:
                result["cli_error"] = r.stderr[-500:]
                break
            line = [l for l in r.stderr.splitlines() if l.startswith('{"animation"')][-1]
            fps.append(json.loads(line)["frames_per_s"])
    result["cli_frames_32_shutter_0.5"] = {"frames_per_s_best_of_3": max(fps) if fps else None, "runs": fps}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result["cli_frames_32_shutter_0.5"]))


if __name__ == "__main__":
    main()
