#!/usr/bin/env python3
"""What progressive rendering costs: the headline frame (cfg2, 1200x800, spp 128) as ONE rt_hip_render against K = 1, 2, 4, 8, 16
passes of rt_hip_accumulate on one stream (contiguous, as even as they come) + one rt_hip_resolve.  GPU machine only.

    python tools/progressive_bench.py [--reps 5]  > profiles/progressive_bench.json

Kernel times are HIP-event times of the launches (rt_hip_wait), medians over --reps repetitions after a warm-up that lets the
queue order settle (both forms share it: same tile geometry).  Prints one JSON line: per K the total kernel time of the passes,
its excess over the one-shot kernel, that excess per extra launch, and the resolve kernel; each final image is checked
bit-identical to the one-shot frame."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scene", default="scenes/cfg2_cover_1200x800_spp128.json")
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    sc = pkg.host.Scene.load(a.scene)
    w, h, spp = sc.c.width, sc.c.height, sc.c.samples_per_pixel
    gs = pkg.hip.HipScene(sc.ptr, 0)
    stream = torch.cuda.current_stream()
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    res = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")

    def one_shot():
        gs.render(rgb.data_ptr(), 0, None, stream.cuda_stream)
        return gs.wait()["kernel_ms"]

    def passes(k):
        acc.zero_()
        ms = []
        b = 0
        for i in range(k):
            n = spp // k + (1 if i < spp % k else 0)
            gs.accumulate(acc.data_ptr(), b, n, None, stream.cuda_stream)
            ms.append(gs.wait()["kernel_ms"])
            b += n
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        gs.resolve(acc.data_ptr(), spp, res.data_ptr(), 0, None, stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return ms, e0.elapsed_time(e1)

    for _ in range(3):   # warm-up: code objects, kernel configurations, the measured queue order
        one_shot()
        passes(2)
    base = statistics.median(one_shot() for _ in range(a.reps))
    want = rgb.cpu().numpy()
    out = {"tool": "progressive_bench", "scene": os.path.basename(a.scene), "width": w, "height": h, "spp": spp, "reps": a.reps,
           "one_shot_kernel_ms": round(base, 4), "passes": []}
    for k in (1, 2, 4, 8, 16):
        runs = [passes(k) for _ in range(a.reps)]
        total = statistics.median(sum(ms) for ms, _ in runs)
        resolve = statistics.median(r for _, r in runs)
        identical = bool(np.array_equal(res.cpu().numpy(), want))
        out["passes"].append({"k": k, "kernel_ms_total": round(total, 4), "excess_ms": round(total - base, 4),
                              "excess_ms_per_extra_launch": round((total - base) / (k - 1), 4) if k > 1 else None,
                              "pass_kernel_ms_median": round(statistics.median(runs[len(runs) // 2][0]), 4),
                              "resolve_ms": round(resolve, 4), "identical_to_one_shot": identical})
        if not identical:
            print(json.dumps(out), flush=True)
            raise SystemExit(f"K = {k}: the resolved frame differs from the one-shot frame")
    gs.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
