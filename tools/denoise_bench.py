#!/usr/bin/env python3
"""What denoising costs and buys: the headline frame (cfg2, 1200x800) and the lit test scene (cfg1, 800x600).
GPU machine only.

    python tools/denoise_bench.py [--reps 7] [--out profiles/denoise_bench.json]

Per scene: rt_aov kernel time for n = 1, 4, 8 and the whole rt_hip_denoise for L = 1 .. 8 (HIP events around each call; median,
min and max over --reps after a warm-up); the RMSE of linear radiance against a --ref-spp one-shot frame of another seed, noisy and
denoised (default iterations and sigmas, AOVs over min(8, spp) samples), at spp 4 .. 128; and the equal-time comparison: denoised at
N spp against a noisy uniform frame at the spp whose megakernel time equals N's kernel + AOV + filter time.  A small sigma sweep at
16 spp shows where the defaults sit.  Pixels that are NaN in either frame are left out of every RMSE."""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--spps", default="4,8,16,32,64,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft

    os.chdir(ROOT)
    pkg = graft.load_package()
    HS = pkg.hip.HipScene
    stream = torch.cuda.current_stream()
    out = {"reference": {"spp": a.ref_spp, "seed": "0x5EED5EED"}, "defaults": {"iterations": HS.DENOISE_ITERATIONS, "sigmas": HS.DENOISE_SIGMAS,
                                                                                "aov_samples": HS.DENOISE_AOV_SAMPLES}, "scenes": []}

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

    for path in ("scenes/cfg2_cover_1200x800_spp128.json", "scenes/cfg1_test_800x600_spp16.json"):
        sc = pkg.host.Scene.load(path)
        w, h = sc.c.width, sc.c.height
        gs = HS(sc.ptr, 0)
        lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        aov = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda:0")
        den = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        drgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")

        def one_shot(spp, scene=gs):
            scene.set_option("samples_per_pixel", spp)
            scene.render(rgb.data_ptr(), lin.data_ptr(), None, stream.cuda_stream)
            return scene.wait()["kernel_ms"]

        def kernel_ms(spp):
            one_shot(spp)
            return statistics.median([one_shot(spp) for _ in range(3)])

        ref_scene = HS(sc.ptr, 0)
        ref_scene.set_option("seed", 0x5EED5EED)
        one_shot(a.ref_spp, ref_scene)
        ref = lin.cpu().numpy().astype(np.float64)
        ref_scene.close()

        def rmse(x):
            x = np.asarray(x, np.float64)
            ok = ~np.isnan(ref).any(-1) & ~np.isnan(x).any(-1)
            return float(np.sqrt(np.mean((x[ok] - ref[ok]) ** 2)))

        def aovs(n):
            gs.render_aovs(n, aov.data_ptr(), stream=stream.cuda_stream)

        def denoise(L=HS.DENOISE_ITERATIONS, sigmas=HS.DENOISE_SIGMAS):
            gs.denoise(lin.data_ptr(), aov.data_ptr(), L, den.data_ptr(), drgb.data_ptr(), sigmas=sigmas, stream=stream.cuda_stream)

        s = {"scene": path, "width": w, "height": h, "aov": {}, "denoise": {}, "rmse": [], "equal_time": [], "sigma_sweep": []}
        for n in (1, 4, 8):
            s["aov"][str(n)] = spread(lambda: aovs(n))
        one_shot(16)
        aovs(8)
        for L in range(1, 9):
            s["denoise"][str(L)] = spread(lambda: denoise(L))
        print(json.dumps({k: s[k] for k in ("scene", "aov", "denoise")}), file=sys.stderr, flush=True)
        t_dn = s["denoise"][str(HS.DENOISE_ITERATIONS)]["median_ms"]
        for N in [int(x) for x in a.spps.split(",")]:
            k_ms = kernel_ms(N)
            noisy = rmse(lin.cpu().numpy())
            n_aov = min(HS.DENOISE_AOV_SAMPLES, N)
            aovs(n_aov)
            denoise()
            torch.cuda.synchronize()
            dn = rmse(den.cpu().numpy())
            s["rmse"].append({"spp": N, "kernel_ms": round(k_ms, 4), "noisy": noisy, "denoised": dn, "ratio": round(dn / noisy, 4)})
            if str(n_aov) not in s["aov"]:
                s["aov"][str(n_aov)] = spread(lambda: aovs(n_aov))
            total = k_ms + s["aov"][str(n_aov)]["median_ms"] + t_dn
            spp_t = max(N, int(round(N * total / k_ms)))
            t_ms = kernel_ms(spp_t)
            s["equal_time"].append({"spp": N, "denoised_total_ms": round(total, 4), "denoised_rmse": dn, "uniform_spp": spp_t,
                                    "uniform_kernel_ms": round(t_ms, 4), "uniform_rmse": rmse(lin.cpu().numpy())})
            print(json.dumps(s["rmse"][-1]), json.dumps(s["equal_time"][-1]), file=sys.stderr, flush=True)
        # repeatability of the RMSE: three seeds at 16 spp, noisy and denoised
        rep = []
        for seed in (1, 2, 3):
            gs.set_option("seed", seed)
            one_shot(16)
            aovs(8)
            denoise()
            torch.cuda.synchronize()
            rep.append({"seed": seed, "noisy": rmse(lin.cpu().numpy()), "denoised": rmse(den.cpu().numpy())})
        gs.set_option("seed", sc.c.seed)
        s["rmse_16spp_other_seeds"] = rep
        one_shot(16)
        aovs(8)
        for L, sc_, sn, sa, sz in itertools.product((1, 2, 3, 5), (0.05, 0.1, 0.25, 0.5, 1.0), (0.1, 0.3, 1.0), (0.02, 0.1, 0.3), (0.01, 0.05, 0.5, 10.0)):
            denoise(L, (sc_, sn, sa, sz))
            torch.cuda.synchronize()
            s["sigma_sweep"].append({"L": L, "sigmas": [sc_, sn, sa, sz], "rmse": rmse(den.cpu().numpy())})
        s["sigma_sweep"].sort(key=lambda r: r["rmse"])
        s["sigma_sweep"] = s["sigma_sweep"][:20]
        print(json.dumps(s["sigma_sweep"][:3]), file=sys.stderr, flush=True)
        gs.close()
        out["scenes"].append(s)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"done": a.out}))


if __name__ == "__main__":
    main()
