#!/usr/bin/env python3
"""What adaptive sampling buys: the headline frame (cfg2, 1200x800, spp 128) rendered by rt_hip_render_adaptive_to_host at a few
thresholds, each against uniform one-shot frames of the same total samples and of the same kernel time.  GPU machine only.

    python tools/adaptive_bench.py [--reps 3] [--out profiles/adaptive_bench.json]

Per threshold: kernel time (sum of the rounds' megakernel launches) and wall time (medians over --reps after a warm-up), rounds,
samples traced, the histogram of tile counts n_t, and the RMSE of linear radiance against a high-spp one-shot reference of the
same scene rendered with another seed (independent noise).  The adaptive frame's linear radiance is assembled tile by tile from
one-shot frames at each n_t, which the exactness contract (tests/test_adaptive.py) makes the same values.  Also
an A/B of the list launch's queue (XCD affinity off, the caller's order) against whole-frame accumulating launches."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", default="scenes/cfg2_cover_1200x800_spp128.json")
    ap.add_argument("--thresholds", default="0,0.01,0.02,0.05")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    sc = pkg.host.Scene.load(a.scene)
    w, h, N = sc.c.width, sc.c.height, sc.c.samples_per_pixel
    stream = torch.cuda.current_stream()
    gs = pkg.hip.HipScene(sc.ptr, 0)
    lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")

    def one_shot(spp, scene=gs):
        scene.set_option("samples_per_pixel", spp)
        scene.render(rgb.data_ptr(), lin.data_ptr(), None, stream.cuda_stream)
        st = scene.wait()
        scene.set_option("samples_per_pixel", N)
        return lin.cpu().numpy().astype(np.float64), st["kernel_ms"]

    ref_scene = pkg.hip.HipScene(sc.ptr, 0)
    ref_scene.set_option("seed", 0x5EED5EED)
    ref, ref_ms = one_shot(a.ref_spp, ref_scene)
    ref_scene.close()

    def rmse(x):
        return float(np.sqrt(np.mean((x - ref) ** 2)))

    one_ms = statistics.median([one_shot(N)[1] for _ in range(a.reps + 2)][2:])
    out = {"scene": a.scene, "width": w, "height": h, "spp": N, "min_spp": a.min_spp, "reference": {"spp": a.ref_spp, "seed": "0x5EED5EED"},
           "one_shot": {"kernel_ms": round(one_ms, 4), "rmse": rmse(one_shot(N)[0])}, "thresholds": []}
    tw, th, tx, ty = gs.tile_grid()
    out["tile"] = [tw, th, tx, ty]
    for E in [float(x) for x in a.thresholds.split(",")]:
        gs.render_adaptive(E, a.min_spp)   # (warm-up)
        runs = [gs.render_adaptive(E, a.min_spp) for _ in range(a.reps)]
        img, n_t, st = runs[-1]
        rounds = gs.adaptive_rounds()
        assert all(np.array_equal(r[1], n_t) and np.array_equal(r[0], img) for r in runs), "not deterministic"
        frame = np.zeros((h, w, 3), np.float64)
        for c in np.unique(n_t):
            f, _ = one_shot(int(c))
            mask = np.kron(n_t == c, np.ones((th, tw), bool))[:h, :w]
            frame[mask] = f[mask]
        spp_eq = max(1, int(round(st["samples"] / (w * h))))
        k_ms = statistics.median(r[2]["kernel_ms"] for r in runs)
        spp_t = max(1, int(round(N * k_ms / one_ms)))
        f_eq, eq_ms = one_shot(spp_eq)
        f_t, t_ms = one_shot(spp_t)
        hist = {str(int(c)): int((n_t == c).sum()) for c in np.unique(n_t)}
        out["thresholds"].append({
            "E": E, "kernel_ms": round(k_ms, 4), "wall_ms": round(statistics.median(r[2]["frame_ms"] for r in runs), 4),
            "rounds": [{"tiles": r[0], "spp": r[1], "kernel_ms": r[2]} for r in rounds], "samples": int(st["samples"]),
            "samples_fraction": round(st["samples"] / (w * h * N), 4), "n_t_histogram": hist, "rmse": rmse(frame),
            "uniform_same_samples": {"spp": spp_eq, "kernel_ms": round(eq_ms, 4), "rmse": rmse(f_eq)},
            "uniform_same_kernel_time": {"spp": spp_t, "kernel_ms": round(t_ms, 4), "rmse": rmse(f_t)}})
        print(json.dumps(out["thresholds"][-1]), file=sys.stderr, flush=True)

    # A/B of the list launch's queue: all tiles of the frame through rt_hip_accumulate_tiles (affinity off, bottom row first) against
    # whole-frame rt_hip_accumulate with XCD affinity on (the default) and off, each on its own scene after three warm-up frames,
    # alternating, [0, N) in one launch
    acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
    nt = tx * ty
    d_list = torch.from_numpy(np.arange(nt - 1, -1, -1, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
    arms = {"whole_affinity_on": pkg.hip.HipScene(sc.ptr, 0), "whole_affinity_off": pkg.hip.HipScene(sc.ptr, 0), "list_all_tiles": pkg.hip.HipScene(sc.ptr, 0)}
    arms["whole_affinity_off"].set_option("tile_affinity", 0)

    def run(name):
        s = arms[name]
        acc.zero_()
        if name == "list_all_tiles":
            s.accumulate_tiles(d_list.data_ptr(), nt, acc.data_ptr(), 0, N, None, stream.cuda_stream)
        else:
            s.accumulate(acc.data_ptr(), 0, N, None, stream.cuda_stream)
        return s.wait()["kernel_ms"]

    times = {k: [] for k in arms}
    for i in range(3 + 2 * a.reps):
        for k in arms:
            ms = run(k)
            if i >= 3:
                times[k].append(ms)
    out["list_launch_ab"] = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}
    for s in arms.values():
        s.close()
    gs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["list_launch_ab"]))


if __name__ == "__main__":
    main()
