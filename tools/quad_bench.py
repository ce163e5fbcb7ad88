#!/usr/bin/env python3
"""What quads cost: three frames, kernel time by HIP events, median of 9 runs alternating in one process —
  1. the headline scene (scenes/cfg2_cover_1200x800_spp128.json): no quad, the kernel it always ran;
  2. the headline scene plus ONE small quad hidden behind the camera: the same paths through the QUADS kernel — the price of the arm (one
     quad test per segment) and of what the QUADS kernels give up (tables in L2 instead of LDS, the general colour map);
  3. the Cornell example (scenes/cornell_spheres_600x600_spp128.json): 17 quads, 3 spheres, lit.
GPU machine only.

    python tools/quad_bench.py [--reps 9] [--parent-lib DIR/librt_hip.so] [--out profiles/quad_bench.json]

--parent-lib: librt_hip.so of the PARENT commit (built beside its own librt_host.so); frame 1 is then also rendered through it in the
same alternation, and frame 2 is compared against that time — the headline before this feature existed.  Without it the comparison is
against frame 1 of this build alone, and the file says so.  Reports Msamples/s and quad tests per segment (every segment tests every
quad: the count of quads)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADLINE = "scenes/cfg2_cover_1200x800_spp128.json"
CORNELL = "scenes/cornell_spheres_600x600_spp128.json"


def hidden_quad(cfg):
    """a 1 mm quad five units BEHIND the camera, facing it: no camera ray and practically no bounce can reach it"""
    cam = cfg["camera"]
    f, a = cam["look_from"], cam["look_at"]
    d = [f[k] - a[k] for k in "xyz"]
    n = sum(x * x for x in d) ** 0.5
    q = [f[k] + 5.0 * x / n for k, x in zip("xyz", d)]
    pt = lambda v: {"x": v[0], "y": v[1], "z": v[2]}
    return {"q": pt(q), "u": pt([0.0, 1e-3, 0.0]), "v": pt([d[2] / n * 1e-3, 0.0, -d[0] / n * 1e-3]), "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_bench.json"))
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
    head = json.load(open(HEADLINE))
    hidden = dict(head, objects=head["objects"] + [hidden_quad(head)])
    cfgs = {"headline": head, "headline_hidden_quad": hidden, "cornell": json.load(open(CORNELL))}
    scenes = {}
    for name, cfg in cfgs.items():
        sc = pkg.host.Scene.loads(json.dumps(cfg))
        gs = pkg.hip.HipScene(sc.ptr, 0, center1=sc.center1(), quads=sc.quads())
        scenes[name] = (sc, gs, torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
    if parent is not None:
        sc = pkg.host.Scene.loads(json.dumps(head))
        scenes["headline_parent_commit"] = (sc, pkg.hip.HipScene(sc.ptr, 0, library=parent), torch.zeros((sc.c.height, sc.c.width, 3), dtype=torch.uint8, device="cuda:0"))
    order = (["headline_parent_commit"] if parent is not None else []) + list(cfgs)

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
                     "msamples_per_s": round(st["samples"] / med / 1e3, 1), "last_kernel": kern[name], "quads": quads, "quad_tests_per_segment": quads,
                     "n_spheres": gs.query("n_spheres"), "lds_tables": gs.query("lds_tables"), "samples": st["samples"], "segments": st["segments"],
                     "segments_per_sample": round(st["segments"] / max(st["samples"], 1), 4), "exact_tests_per_segment": round(st["exact_tests"] / seg, 4),
                     "grid_steps_per_segment": round(st["grid_steps"] / seg, 4)}
    base = "headline_parent_commit" if parent is not None else "headline"
    out = {"reps": a.reps, "scenes": {"headline": HEADLINE, "headline_hidden_quad": HEADLINE + " + one hidden quad", "cornell": CORNELL},
           "parent_lib": bool(parent is not None), "compared_against": base, "runs": res,
           "hidden_quad_over_headline_median": round(res["headline_hidden_quad"]["kernel_ms_median"] / res[base]["kernel_ms_median"], 4),
           "headline_over_parent_median": round(res["headline"]["kernel_ms_median"] / res[base]["kernel_ms_median"], 4)}
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for _, gs, _ in scenes.values():
        gs.close()


if __name__ == "__main__":
    main()
