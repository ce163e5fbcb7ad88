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
left out of every RMSE.

    python tools/temporal_bench.py --surface [--out profiles/temporal_surface_bench.json]

The same protocol for the mode with surface tracking, on four animations: the two scenes above, the cover without mirrors
and glass (scenes/cover_diffuse_1200x800_spp128.json), and scenes/cover_motion_1200x800_spp128.json with its spheres moved from frame to
frame as the CLI's --shutter 0.5 moves them.  Columns: raw, per-frame `--denoise`, the mode above with the library's defaults, the surface
mode (RT_TEMPORAL_SURFACE_*, and the best point of a sweep over alpha_min, alpha_specular and n_max scored as above over the four
animations); the last frame of each split by the first hit's material, read from the surface record's `kind`.  rt_surface and
rt_reproject_surface are timed next to rt_aov and rt_reproject in the same process."""
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


SURFACE_SWEEP = {"alpha_min": (0.05, 0.1, 0.2, 0.35, 0.5, 0.65, 0.8), "alpha_specular": (0.35, 0.5, 0.75, 1.0), "n_max": (4.0, 8.0, 32.0)}
SURFACE_CASES = (("cover", "scenes/cfg2_cover_1200x800_spp128.json", False), ("test", "scenes/cfg1_test_800x600_spp16.json", False),
                 ("diffuse", "scenes/cover_diffuse_1200x800_spp128.json", False), ("moving", "scenes/cover_motion_1200x800_spp128.json", True))
SURFACE_KINDS = {0: "lambertian", 1: "metal", 2: "glass", 3: "texture", 4: "light", 5: "medium", 6: "checker", 7: "noise", 0xFFFFFFFF: "sky"}
SHUTTER = 0.5


def dump_compact(obj, f, width=240, digits=6):
    """json with one key per line, except that a list or map of numbers, and any value whose compact form fits `width` characters, stays on one
    line; floats rounded to `digits` decimals (the per-frame tables are long and are read by programs)"""
    def rnd(o):
        if isinstance(o, float):
            return round(o, digits)
        if isinstance(o, dict):
            return {k: rnd(v) for k, v in o.items()}
        return [rnd(v) for v in o] if isinstance(o, (list, tuple)) else o

    def emit(o, depth):
        flat = json.dumps(o, separators=(", ", ": "))
        scalars = isinstance(o, (list, dict)) and all(not isinstance(v, (list, dict)) for v in (o.values() if isinstance(o, dict) else o))
        if not isinstance(o, (list, dict)) or scalars or len(flat) <= width or not o:
            return flat
        pad, end = "\n" + " " * (depth + 1), "\n" + " " * depth
        if isinstance(o, dict):
            return "{" + ",".join(pad + json.dumps(k) + ": " + emit(v, depth + 1) for k, v in o.items()) + end + "}"
        return "[" + ",".join(pad + emit(v, depth + 1) for v in o) + end + "]"
    f.write(emit(rnd(obj), 0) + "\n")


def surface_main(a):
    """--surface: profiles/temporal_surface_bench.json"""
    import numpy as np
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    HS = pkg.hip.HipScene
    stream = torch.cuda.current_stream()
    taus = HS.TEMPORAL_PARAMS[2:]
    lib_surface = {"alpha_min": HS.TEMPORAL_SURFACE_PARAMS[0], "alpha_specular": HS.TEMPORAL_SURFACE_PARAMS[1], "n_max": HS.TEMPORAL_PARAMS[1]}
    grid = [dict(zip(SURFACE_SWEEP, p)) for p in itertools.product(*SURFACE_SWEEP.values())]
    point_key = lambda p: "%g/%g/%g" % (p["alpha_min"], p["alpha_specular"], p["n_max"])
    out = {"animation": {"frames": a.frames, "orbit_deg_per_frame": a.orbit, "shutter_of_the_moving_case": SHUTTER}, "reference": {"spp": a.ref_spp, "seed": "0x5EED5EED"},
           "temporal_defaults": dict(zip(SWEEP, HS.TEMPORAL_PARAMS)), "surface_defaults": lib_surface, "thresholds": dict(zip(("tau_n", "tau_a", "tau_z"), taus)),
           "spatial": {"iterations": HS.DENOISE_ITERATIONS, "sigmas": HS.DENOISE_SIGMAS}, "sweep_grid": {k: list(v) for k, v in SURFACE_SWEEP.items()},
           "sweep_spp": a.sweep_spp, "steady_from_frame": STEADY_FROM, "cases": []}
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
    mean_from = lambda v: float(sum(v[STEADY_FROM:]) / max(1, len(v[STEADY_FROM:])))
    set_cam = lambda scene, c: scene.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])

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

    def rmse_by_kind(x, ref, kind):
        x, ref = x.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
        ok = ~(np.isnan(x).any(-1) | np.isnan(ref).any(-1))
        res = {}
        for k in np.unique(kind):
            m = ok & (kind == k)
            if m.any():
                res[SURFACE_KINDS.get(int(k), str(int(k)))] = {"share": round(float(m.mean()), 4), "rmse": float(np.sqrt(np.mean((x[m] - ref[m]) ** 2)))}
        return res

    def make_steps(gs, cams, lins, aovs, surfs, refs, disps, hist, empty_h, empty_a, empty_s, packed, den):
        """(chain, step18, step19) over one animation's frames (a factory: the best point's tables are made after every case has run)"""
        def chain(step, t_only=None, last=None):
            """the animation through one of the two steps + the spatial filter: per-frame RMSE of what leaves"""
            prev, res = None, []
            for f in range(a.frames):
                set_cam(gs, cams[f])
                o = hist[f & 1]
                step(f, prev, o)
                packed.copy_(o[..., 0:3])
                if t_only is not None:
                    t_only.append(rmse(packed, refs[f]))
                gs.denoise(packed.data_ptr(), aovs[f].data_ptr(), HS.DENOISE_ITERATIONS, den.data_ptr(), 0, stream=stream.cuda_stream)
                res.append(rmse(den, refs[f]))
                prev = (o, f)
            if last is not None:
                last["temporal"], last["temporal_spatial"] = packed.clone(), den.clone()
            return res

        def step18(params):
            def step(f, prev, o):
                ph, pa, pc = (empty_h, aovs[0], cams[0]) if prev is None else (prev[0], aovs[f - 1], cams[f - 1])
                gs.reproject(lins[f].data_ptr(), aovs[f].data_ptr(), ph.data_ptr(), pa.data_ptr(), pc, o.data_ptr(), params, stream=stream.cuda_stream)
            return step

        def step19(p):
            params = (p["alpha_min"], p["n_max"]) + tuple(taus)

            def step(f, prev, o):
                ph, pa, ps, pc = (empty_h, empty_a, empty_s, cams[0]) if prev is None else (prev[0], aovs[f - 1], surfs[f - 1], cams[f - 1])
                d = disps[f]
                gs.reproject_surface(lins[f].data_ptr(), aovs[f].data_ptr(), surfs[f].data_ptr(), ph.data_ptr(), pa.data_ptr(), ps.data_ptr(), pc, o.data_ptr(),
                                     d_displacement=0 if d is None else d.data_ptr(), params=params, alpha_specular=p["alpha_specular"], stream=stream.cuda_stream)
            return step

        return chain, step18, step19

    sweep_scores = []
    keep = []
    for name, path, moving in SURFACE_CASES:
        sc = pkg.host.Scene.load(path)
        w, h, n = sc.c.width, sc.c.height, sc.c.n_spheres
        cams = orbit_cameras(pkg, json.load(open(path))["camera"], a.frames, a.orbit)
        c0 = np.array([[sc.c.spheres[i].center[k] for k in range(3)] for i in range(n)], np.float64)
        if moving:   # rust-raytracer_amd/csrc/host/anim_path.h: the spheres of frame f
            dv = np.array(sc.center1(), np.float64).reshape(-1, 3) - c0
            centres = [(c0 + dv * (np.float64(f) / a.frames), c0 + dv * ((np.float64(f) + SHUTTER) / a.frames)) for f in range(a.frames)]
            mids = [c + (c1 - c) * 0.5 for c, c1 in centres]
            disps = [torch.from_numpy(np.zeros_like(c0) if f == 0 else mids[f] - mids[f - 1]).to("cuda:0") for f in range(a.frames)]
            make = lambda: HS(sc.ptr, 0, center1=centres[0][1])
        else:
            centres, disps, make = None, [None] * a.frames, lambda: HS(sc.ptr, 0)
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        refs = []
        ref_scene = make()
        ref_scene.set_option("seed", 0x5EED5EED)
        ref_scene.set_option("samples_per_pixel", a.ref_spp)
        for f, c in enumerate(cams):
            set_cam(ref_scene, c)
            if moving:
                ref_scene.update_spheres(*centres[f])
            r = f32(h, w, 3)
            ref_scene.render(rgb.data_ptr(), r.data_ptr(), None, stream.cuda_stream)
            ref_scene.wait()
            refs.append(r)
        ref_scene.close()
        gs = make()
        case = {"case": name, "scene": path, "width": w, "height": h, "spheres_move": moving, "runs": []}
        acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
        hist, empty_h, empty_a = [f32(h, w, 4), f32(h, w, 4)], f32(h, w, 4), f32(h, w, 8)
        empty_s = torch.zeros((h, w, 2), dtype=torch.int64, device="cuda:0")
        packed, den = f32(h, w, 3), f32(h, w, 3)
        for spp in [int(x) for x in a.spps.split(",")]:
            gs.set_option("samples_per_pixel", spp)
            lins, aovs, surfs, kernel_ms = [], [], [], []
            for f, c in enumerate(cams):
                set_cam(gs, c)
                if moving:
                    gs.update_spheres(*centres[f])
                acc.zero_()
                gs.accumulate(acc.data_ptr(), f * spp, spp, stream=stream.cuda_stream)
                kernel_ms.append(gs.wait()["kernel_ms"])
                lin, aov, surf = f32(h, w, 3), f32(h, w, 8), torch.zeros((h, w, 2), dtype=torch.int64, device="cuda:0")
                gs.resolve(acc.data_ptr(), spp, 0, lin.data_ptr(), stream=stream.cuda_stream)
                gs.render_aovs(min(HS.DENOISE_AOV_SAMPLES, spp), aov.data_ptr(), stream=stream.cuda_stream)
                gs.render_surface(surf.data_ptr(), stream=stream.cuda_stream)
                lins.append(lin)
                aovs.append(aov)
                surfs.append(surf)
            torch.cuda.synchronize()
            raw = [rmse(lins[f], refs[f]) for f in range(a.frames)]
            spatial = []
            for f in range(a.frames):
                gs.denoise(lins[f].data_ptr(), aovs[f].data_ptr(), HS.DENOISE_ITERATIONS, den.data_ptr(), 0, stream=stream.cuda_stream)
                spatial.append(rmse(den, refs[f]))
            last_spatial = den.clone()

            chain, step18, step19 = make_steps(gs, cams, lins, aovs, surfs, refs, disps, hist, empty_h, empty_a, empty_s, packed, den)

            run = {"spp": spp, "megakernel_ms_per_frame": round(statistics.median(kernel_ms), 4), "raw": raw, "spatial": spatial,
                   "steady_means": {"raw": mean_from(raw), "spatial": mean_from(spatial)}}
            kind = surfs[-1].cpu().numpy().view(np.uint32)[..., 1]
            by_kind = {"raw": rmse_by_kind(lins[-1], refs[-1], kind), "spatial": rmse_by_kind(last_spatial, refs[-1], kind)}
            for key, step in (("temporal_defaults", step18(HS.TEMPORAL_PARAMS)), ("surface_defaults", step19(lib_surface))):
                t_only, last = [], {}
                ts = chain(step, t_only, last)
                run[key] = {"temporal_spatial": ts, "temporal": t_only}
                run["steady_means"][key] = {"temporal": mean_from(t_only), "temporal_spatial": mean_from(ts)}
                by_kind[key] = {"temporal": rmse_by_kind(last["temporal"], refs[-1], kind), "temporal_spatial": rmse_by_kind(last["temporal_spatial"], refs[-1], kind)}
            run["last_frame_by_first_hit"] = by_kind
            # the four kernels in one process: frame 1 onto frame 0's history (n' = 1 at every pixel), the scene's tables and camera of the last frame
            set_cam(gs, cams[0])
            step19(lib_surface)(0, None, hist[0])
            set_cam(gs, cams[1])
            n_aov = min(HS.DENOISE_AOV_SAMPLES, spp)
            run["kernels_ms"] = {
                "rt_aov": spread(lambda: gs.render_aovs(n_aov, empty_a.data_ptr(), stream=stream.cuda_stream)),
                "rt_surface": spread(lambda: gs.render_surface(empty_s.data_ptr(), stream=stream.cuda_stream)),
                "rt_reproject": spread(lambda: step18(HS.TEMPORAL_PARAMS)(1, (hist[0], 0), hist[1])),
                "rt_reproject_surface": spread(lambda: step19(lib_surface)(1, (hist[0], 0), hist[1]))}
            torch.cuda.synchronize()
            run["reproject_surface_history_share"] = round(float((hist[1][..., 3] > 1.0).float().mean().item()), 4)
            empty_a.zero_()
            empty_s.zero_()
            if spp == a.sweep_spp:
                scores = [mean_from(chain(step19(p))) / mean_from(raw) for p in grid]
                sweep_scores.append(scores)
                order = sorted(range(len(grid)), key=lambda i: scores[i])
                run["sweep"] = {point_key(grid[i]): round(scores[i], 5) for i in order}   # "alpha_min/alpha_specular/n_max": score, best first
                run["sweep_scores_of_the_columns"] = {"spatial": round(mean_from(spatial) / mean_from(raw), 5),
                                                      "temporal_defaults": round(run["steady_means"]["temporal_defaults"]["temporal_spatial"] / mean_from(raw), 5)}
                keep.append((run, chain, step19, rmse_by_kind, refs, kind))
            print(json.dumps({"case": name, "spp": spp, "kernels_ms": run["kernels_ms"], "steady_means": run["steady_means"],
                              "last_frame_by_first_hit": by_kind}), file=sys.stderr, flush=True)
            case["runs"].append(run)
        case["_gs"] = gs
        out["cases"].append(case)
    if sweep_scores:
        combined = [sum(sc_[i] for sc_ in sweep_scores) / len(sweep_scores) for i in range(len(grid))]
        order = sorted(range(len(grid)), key=lambda i: combined[i])
        out["best"] = dict(grid[order[0]], score=round(combined[order[0]], 5))
        out["sweep_combined"] = {point_key(grid[i]): round(combined[i], 5) for i in order}
        print(json.dumps({"best": out["best"]}), file=sys.stderr, flush=True)
        for run, chain, step19, by_kind_fn, refs, kind in keep:   # the best point's own tables, per case at the sweep's spp
            t_only, last = [], {}
            ts = chain(step19(grid[order[0]]), t_only, last)
            run["best_point"] = {"temporal_spatial": ts, "temporal": t_only}
            run["steady_means"]["best_point"] = {"temporal": mean_from(t_only), "temporal_spatial": mean_from(ts)}
            run["last_frame_by_first_hit"]["best_point"] = {"temporal": by_kind_fn(last["temporal"], refs[-1], kind),
                                                            "temporal_spatial": by_kind_fn(last["temporal_spatial"], refs[-1], kind)}
    for case in out["cases"]:
        case.pop("_gs").close()
    with open(a.out, "w") as f:
        dump_compact(out, f)
    print(json.dumps({"done": a.out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--orbit", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--spps", default="8,16")
    ap.add_argument("--sweep-spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--surface", action="store_true", help="the mode with surface tracking (DESIGN.md §19): profiles/temporal_surface_bench.json")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "temporal_surface_bench.json" if a.surface else "temporal_bench.json")
    if a.surface:
        return surface_main(a)
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
