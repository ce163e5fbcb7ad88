#!/usr/bin/env python3
"""What temporal denoising costs and buys: a 32-frame orbit of 3 degrees per frame over the headline scene (cfg2,
1200x800) and the lit test scene (cfg1, 800x600), at 8 and 16 spp.  GPU machine only.

    python tools/temporal_bench.py [--frames 32] [--orbit 3] [--reps 7] [--out profiles/temporal_bench.json]

Per scene and spp, per frame: the RMSE of linear radiance against a --ref-spp one-shot frame of another seed at the same camera, for
the raw frame (samples [f spp, (f + 1) spp), what the temporal mode traces), the raw frame through the spatial filter alone
(`--denoise` per frame: default iterations and sigmas), the temporal history, and the history through the spatial filter (what the
temporal mode writes).  The HIP-event time of rt_reproject (median, min, max over --reps after a warm-up) and of a frame's megakernel.
A sweep over alpha_min, n_max and the three thresholds at 16 spp — scored by the mean over frames 8 .. of the temporal + spatial RMSE
relative to the raw frames', averaged over the two scenes — names the point the header's RT_TEMPORAL_* defaults are taken from; the
per-frame tables are recorded for that point, for the defaults the library was built with and for FIRST_GUESS, the parameters before
any sweep.  rt_reproject is timed on frame 1 against frame 0's real history and guides.  Pixels that are NaN in either frame are
left out of every RMSE."""
import argparse
import itertools
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP = {"alpha_min": (0.05, 0.1, 0.2, 0.35, 0.5), "n_max": (8.0, 32.0), "tau_n": (0.02, 0.1, 0.5), "tau_a": (0.003, 0.01, 0.05, 0.3),
         "tau_z": (0.02, 0.1, 0.5)}
FIRST_GUESS = (0.1, 32.0, 0.05, 0.02, 0.1)   # alpha_min, n_max, tau_n, tau_a, tau_z before any sweep: recorded beside the library's defaults
STEADY_FROM = 8   # frames before this one are the history's warm-up: they are recorded, not scored


def orbit_cameras(pkg, cam, frames, deg):
    """the scene file's camera turned about vup around look_at by deg per frame (the CLI's --orbit), 12 doubles per frame"""
    import numpy as np
    v = lambda k: np.array([cam[k]["x"], cam[k]["y"], cam[k]["z"]], np.float64)
    lf, la, up = v("look_from"), v("look_at"), v("vup")
    k = up / np.linalg.norm(up)
    out = []
    for f in range(frames):
        th = math.radians(deg * f)
        d = lf - la
        frm = la + d * math.cos(th) + np.cross(k, d) * math.sin(th) + k * float(k @ d) * (1.0 - math.cos(th))
        c = pkg.host.camera_derive(list(frm), list(la), list(up), cam["vfov"], cam["aspect"])
        out.append(c["origin"] + c["lower_left_corner"] + c["horizontal"] + c["vertical"])
    return out


KINDS = {0: "lambertian", 1: "metal", 2: "glass", 4: "light"}   # include/rt_abi.h RT_MAT_*


def first_hit_classes(sc, aov):
    """what each pixel shows, read off the guides: "sky" (coverage 0), the material kind of the sphere whose albedo the pixel's albedo
    equals (full coverage; Glass and Light report (1, 1, 1)), "other" (textures, partly covered pixels, albedos two kinds share)"""
    import numpy as np
    kind_of = {}
    for i in range(sc.c.n_spheres):
        sp = sc.c.spheres[i]
        name = KINDS.get(int(sp.kind))
        key = (1.0, 1.0, 1.0) if name in ("glass", "light") else tuple(float(np.float32(sp.albedo[k])) for k in range(3))
        if name:
            kind_of[key] = name if kind_of.get(key, name) == name else "other"
    a = aov.cpu().numpy()
    cls = np.full(a.shape[:2], "other", dtype=object)
    cls[a[..., 7] == 0.0] = "sky"
    full = a[..., 7] == 1.0
    colours, inverse = np.unique(a[full][:, 0:3], axis=0, return_inverse=True)
    names = np.array([kind_of.get(tuple(float(x) for x in c), "other") for c in colours], dtype=object)
    cls[full] = names[inverse.reshape(-1)]
    return cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--orbit", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--spps", default="8,16")
    ap.add_argument("--sweep-spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.json"))
    a = ap.parse_args()
    import numpy as np  # noqa: F401
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    HS = pkg.hip.HipScene
    stream = torch.cuda.current_stream()
    grid = [dict(zip(SWEEP, p)) for p in itertools.product(*SWEEP.values())]
    as_tuple = lambda d: (d["alpha_min"], d["n_max"], d["tau_n"], d["tau_a"], d["tau_z"])
    out = {"animation": {"frames": a.frames, "orbit_deg_per_frame": a.orbit}, "reference": {"spp": a.ref_spp, "seed": "0x5EED5EED"},
           "library_defaults": dict(zip(SWEEP, HS.TEMPORAL_PARAMS)), "first_guess": dict(zip(SWEEP, FIRST_GUESS)), "spatial": {"iterations": HS.DENOISE_ITERATIONS, "sigmas": HS.DENOISE_SIGMAS},
           "sweep_grid": {k: list(v) for k, v in SWEEP.items()}, "sweep_spp": a.sweep_spp, "steady_from_frame": STEADY_FROM, "scenes": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def spread(fn):
        fn()
        v = [timed(fn) for _ in range(a.reps)]
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def rmse(x, ref):
        ok = ~(torch.isnan(ref).any(-1) | torch.isnan(x).any(-1))
        d = (x.double() - ref.double())[ok]
        return float(torch.sqrt((d * d).mean()).item())

    def rmse_by_class(x, ref, cls):
        """RMSE over the pixels of each class, with the class's share of the frame"""
        import numpy as np
        x, ref = x.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
        ok = ~(np.isnan(x).any(-1) | np.isnan(ref).any(-1))
        res = {}
        for name in sorted(set(cls.reshape(-1))):
            m = ok & (cls == name)
            if m.any():
                res[name] = {"share": round(float(m.mean()), 4), "rmse": float(np.sqrt(np.mean((x[m] - ref[m]) ** 2)))}
        return res

    def make_chain(gs, cams, lins, aovs, refs):
        h, w = gs.height, gs.width
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
        hist, empty, packed, den = [f32(h, w, 4), f32(h, w, 4)], f32(h, w, 4), f32(h, w, 3), f32(h, w, 3)

        def chain(params, temporal_only=None, last=None):
            """the animation through rt_hip_reproject + the spatial filter: per-frame RMSE of what leaves (last: a dict that receives the
            last frame's history and filtered history)"""
            prev_h, prev_a, prev_c = empty, aovs[0], cams[0]
            res = []
            for f in range(len(cams)):
                c = cams[f]
                gs.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
                o = hist[f & 1]
                gs.reproject(lins[f].data_ptr(), aovs[f].data_ptr(), prev_h.data_ptr(), prev_a.data_ptr(), prev_c, o.data_ptr(), params,
                             stream=stream.cuda_stream)
                packed.copy_(o[..., 0:3])
                if temporal_only is not None:
                    temporal_only.append(rmse(packed, refs[f]))
                gs.denoise(packed.data_ptr(), aovs[f].data_ptr(), HS.DENOISE_ITERATIONS, den.data_ptr(), 0, stream=stream.cuda_stream)
                res.append(rmse(den, refs[f]))
                prev_h, prev_a, prev_c = o, aovs[f], c
            if last is not None:
                last["temporal"], last["temporal_spatial"] = packed.clone(), den.clone()
            return res
        return chain

    sweep_scores = []   # per scene: the grid's scores
    for path in ("scenes/cfg2_cover_1200x800_spp128.json", "scenes/cfg1_test_800x600_spp16.json"):
        sc = pkg.host.Scene.load(path)
        w, h = sc.c.width, sc.c.height
        cams = orbit_cameras(pkg, json.load(open(path))["camera"], a.frames, a.orbit)
        set_cam = lambda scene, c: scene.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        refs = []
        ref_scene = HS(sc.ptr, 0)
        ref_scene.set_option("seed", 0x5EED5EED)
        ref_scene.set_option("samples_per_pixel", a.ref_spp)
        for c in cams:
            set_cam(ref_scene, c)
            r = f32(h, w, 3)
            ref_scene.render(rgb.data_ptr(), r.data_ptr(), None, stream.cuda_stream)
            ref_scene.wait()
            refs.append(r)
        ref_scene.close()
        gs = HS(sc.ptr, 0)
        s = {"scene": path, "width": w, "height": h, "runs": []}
        acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
        hist, den = [f32(h, w, 4), f32(h, w, 4)], f32(h, w, 3)
        for spp in [int(x) for x in a.spps.split(",")]:
            gs.set_option("samples_per_pixel", spp)
            lins, aovs, kernel_ms = [], [], []
            for f, c in enumerate(cams):   # what the temporal mode traces for frame f, and the guides of its view
                set_cam(gs, c)
                acc.zero_()
                gs.accumulate(acc.data_ptr(), f * spp, spp, stream=stream.cuda_stream)
                kernel_ms.append(gs.wait()["kernel_ms"])
                lin, aov = f32(h, w, 3), f32(h, w, 8)
                gs.resolve(acc.data_ptr(), spp, 0, lin.data_ptr(), stream=stream.cuda_stream)
                gs.render_aovs(min(HS.DENOISE_AOV_SAMPLES, spp), aov.data_ptr(), stream=stream.cuda_stream)
                lins.append(lin)
                aovs.append(aov)
            torch.cuda.synchronize()
            raw = [rmse(lins[f], refs[f]) for f in range(a.frames)]
            spatial = []
            for f in range(a.frames):
                gs.denoise(lins[f].data_ptr(), aovs[f].data_ptr(), HS.DENOISE_ITERATIONS, den.data_ptr(), 0, stream=stream.cuda_stream)
                spatial.append(rmse(den, refs[f]))

            chain = make_chain(gs, cams, lins, aovs, refs)

            mean_from = lambda v: float(sum(v[STEADY_FROM:]) / max(1, len(v[STEADY_FROM:])))
            run = {"spp": spp, "megakernel_ms_per_frame": round(statistics.median(kernel_ms), 4), "raw": raw, "spatial": spatial}
            # rt_reproject's time: frame 1 onto frame 0's real history (n' = 1 at every pixel) and guides, across the 3 degree turn —
            # with the library's defaults, and with thresholds that accept every tap inside the frame (the most work a pixel can do)
            set_cam(gs, cams[0])
            gs.reproject(lins[0].data_ptr(), aovs[0].data_ptr(), hist[1].data_ptr(), aovs[0].data_ptr(), cams[0], hist[0].data_ptr(), HS.TEMPORAL_PARAMS,
                         stream=stream.cuda_stream)   # (hist[1] is all zero: no history; hist[0] becomes frame 0's)
            set_cam(gs, cams[1])
            for key, params in (("reproject", HS.TEMPORAL_PARAMS), ("reproject_all_taps", (HS.TEMPORAL_PARAMS[0], HS.TEMPORAL_PARAMS[1], 1e30, 1e30, 1e30))):
                run[key + "_ms"] = spread(lambda: gs.reproject(lins[1].data_ptr(), aovs[1].data_ptr(), hist[0].data_ptr(), aovs[0].data_ptr(), cams[0],
                                                               hist[1].data_ptr(), params, stream=stream.cuda_stream))
                torch.cuda.synchronize()
                run[key + "_history_share"] = round(float((hist[1][..., 3] > 1.0).float().mean().item()), 4)   # pixels that found history
            hist[1].zero_()
            cls = first_hit_classes(sc, aovs[-1])   # where the error sits in the last frame: diffuse surfaces against mirrors and lenses
            gs.denoise(lins[-1].data_ptr(), aovs[-1].data_ptr(), HS.DENOISE_ITERATIONS, den.data_ptr(), 0, stream=stream.cuda_stream)
            run["last_frame_by_first_hit"] = {"raw": rmse_by_class(lins[-1], refs[-1], cls), "spatial": rmse_by_class(den, refs[-1], cls)}
            run["steady_means"] = {"raw": mean_from(raw), "spatial": mean_from(spatial)}
            for key, params in (("first_guess", FIRST_GUESS), ("library_defaults", HS.TEMPORAL_PARAMS)):
                t_only, last = [], {}
                run[key] = {"temporal_spatial": chain(params, t_only, last), "temporal": t_only}
                run["steady_means"][key] = {"temporal": mean_from(t_only), "temporal_spatial": mean_from(run[key]["temporal_spatial"])}
                run["last_frame_by_first_hit"][key] = {"temporal": rmse_by_class(last["temporal"], refs[-1], cls),
                                                       "temporal_spatial": rmse_by_class(last["temporal_spatial"], refs[-1], cls)}
            if spp == a.sweep_spp:
                scores = [mean_from(chain(as_tuple(p))) / mean_from(raw) for p in grid]
                sweep_scores.append(scores)
                order = sorted(range(len(grid)), key=lambda i: scores[i])
                run["sweep_top"] = [dict(grid[i], score=round(scores[i], 5)) for i in order[:20]]
                run["sweep_worst"] = [dict(grid[i], score=round(scores[i], 5)) for i in order[-3:]]
            print(json.dumps({"scene": path, "spp": spp, "megakernel_ms_per_frame": run["megakernel_ms_per_frame"], "reproject_ms": run["reproject_ms"],
                              "reproject_history_share": run["reproject_history_share"], "reproject_all_taps_ms": run["reproject_all_taps_ms"],
                              "reproject_all_taps_history_share": run["reproject_all_taps_history_share"], "steady_means": run["steady_means"],
                              "last_frame_by_first_hit": run["last_frame_by_first_hit"]}), file=sys.stderr, flush=True)
            s["runs"].append(run)
        s["_chain"] = (gs, chain)   # (the last spp's: the best point is only known after both scenes, its table is made below)
        out["scenes"].append(s)
    if sweep_scores:
        combined = [sum(sc_[i] for sc_ in sweep_scores) / len(sweep_scores) for i in range(len(grid))]
        best = min(range(len(grid)), key=lambda i: combined[i])
        out["best"] = dict(grid[best], score=round(combined[best], 5))
        out["sweep_combined_top"] = [dict(grid[i], score=round(combined[i], 5)) for i in sorted(range(len(grid)), key=lambda i: combined[i])[:20]]
        print(json.dumps({"best": out["best"]}), file=sys.stderr, flush=True)
    for s in out["scenes"]:
        gs, chain = s.pop("_chain")
        if sweep_scores and s["runs"][-1]["spp"] == a.sweep_spp:
            t_only = []
            ts = chain(as_tuple(grid[best]), t_only)
            s["runs"][-1]["best_point"] = {"temporal_spatial": ts, "temporal": t_only}
        gs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"done": a.out}))


if __name__ == "__main__":
    main()
