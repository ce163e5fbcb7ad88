"""Participating media through the layers above the kernel, on the GPU: every one of the 64 MEDIUM instantiations is
selected and launched, an adaptive frame's tiles, a 3-rank emulated group (views sharing the resident density table) and the CLI's
modes each give the one-shot frame bit for bit — on the example scene scenes/cover_fog_1200x800_spp128.json."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_kernel_matrix import ALL_KEYS, CELLS, WIDE, _cell_id, _cell_json, _key
from test_medium_gpu import ACCUM, LENS, MEDIUM, MOTION, _hip_scene, _load, _med, _one_shot, _same, _stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOG = os.path.join(ROOT, "scenes", "cover_fog_1200x800_spp128.json")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _fog_cfg(w, h, spp, lens=False, moving=False):
    cfg = json.load(open(FOG))
    cfg.update(width=w, height=h, samples_per_pixel=spp)
    if lens:
        cfg["camera"].update(aperture=0.2, focus_dist=10.0)
    if moving:   # the smoke ball drifts, and every fourth small sphere bounces
        for i, o in enumerate(cfg["objects"]):
            if ("Medium" in o["material"] and o["radius"] == 1.0) or (o["radius"] == 0.2 and i % 4 == 0):
                c = o["center"]
                o["center1"] = {"x": c["x"] + 0.2, "y": c["y"] + 0.25, "z": c["z"]}
    return cfg


# One scene per cell of the MEDIUM sweep, in the sweep's order: (lights, colour map, LDS / L2 tables) x pinhole / lens x static / moving.
SWEEP_CELLS = [(hl, simple, form, with_lens, moving) for hl, simple, form in CELLS if form != "wide"     # (media with wide tables are refused,
               for with_lens in (False, True) for moving in (False, True)]                                #  test_medium_gpu.py)
SWEEP_KEYS = {MEDIUM | m | l | k for k in ALL_KEYS if not k & WIDE for m in (0, MOTION) for l in (0, LENS)}   # the 64 MEDIUM instantiations


def sweep_name(cell):
    return _cell_id(cell[:3]) + ("/lens" if cell[3] else "") + ("/moving" if cell[4] else "")


def sweep_key(cell):
    """last_kernel of a cell's one-shot frame"""
    return MEDIUM | (MOTION if cell[4] else 0) | (LENS if cell[3] else 0) | _key(*cell[:3])


def sweep_world(host, cell, width, height, pinhole=False):
    """(host scene, center1, lens, number of media) of one cell at width x height, spp 2: the cell's world of test_kernel_matrix.py with
    every third sphere a medium; moving: every second sphere moves over the shutter.  pinhole: the same world without the cell's lens."""
    hl, simple, form, with_lens, moving = cell
    cfg = json.loads(_cell_json(hl, simple, form, width=width, height=height, spp=2))
    rng = np.random.default_rng(2 * SWEEP_CELLS.index(cell))
    n_media = 0
    for i, o in enumerate(cfg["objects"]):
        if i == 0 or "Light" in o["material"]:
            continue
        if i % 3 == 1:
            o["material"] = _med([0.8, 0.7, 0.6], round(float(rng.uniform(1.0, 10.0)), 3))
            n_media += 1
        if moving and i % 2 == 0:
            cc, off = o["center"], rng.uniform(-0.3, 0.3, 3)
            o["center1"] = {"x": cc["x"] + off[0], "y": cc["y"] + off[1], "z": cc["z"] + off[2]}
    if with_lens and not pinhole:
        cfg["camera"].update(aperture=0.5, focus_dist=7.0)
    sc, c1, lens = _load(host, cfg, width, height, 2, cfg["max_depth"])
    return sc, c1, lens, n_media


def test_every_medium_instantiation_is_launched(pkg, abi, host, torch_cuda):
    """(lights, colour map, LDS / L2 tables) x pinhole / lens x static / moving x one-shot / accumulating: the 64 MEDIUM instantiations,
    each selected by the scene that should reach it; the accumulated frame is the one-shot's, and the grid walk is the full scan's.
    (tests/test_feature_matrix.py compares every one of these cells with the restatement.)"""
    torch = torch_cuda
    seen = {}
    for cell in SWEEP_CELLS:
        name = sweep_name(cell)
        sc, c1, lens, n_media = sweep_world(host, cell, 9, 6)
        gs = _hip_scene(pkg, sc, c1, lens)
        assert gs.query("media") == n_media > 0
        want = sweep_key(cell)
        one = _one_shot(torch, gs)
        assert gs.query("last_kernel") == want, (name, gs.query("last_kernel"), want)
        seen.setdefault(want, name)
        acc = torch.zeros((gs.height, gs.width, 3), dtype=torch.int64, device="cuda:0")
        segs = 0
        for b, e in ((1, 2), (0, 1)):
            gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
            segs += gs.wait()["segments"]
        assert gs.query("last_kernel") == want | ACCUM, (name, gs.query("last_kernel"))
        seen.setdefault(want | ACCUM, name)
        rgb = torch.zeros((gs.height, gs.width, 3), dtype=torch.uint8, device="cuda:0")
        lin = torch.zeros((gs.height, gs.width, 3), dtype=torch.float32, device="cuda:0")
        gs.resolve(acc.data_ptr(), 2, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
        torch.cuda.current_stream().synchronize()
        _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), f"{name}: accumulated vs one-shot")
        assert segs == one[2]["segments"], name
        gs.set_option("variant", 1)
        full = _one_shot(torch, gs)
        _same(one, full, f"{name}: grid walk vs full scan")
        assert full[2]["segments"] == one[2]["segments"], name
        gs.close()
    want = SWEEP_KEYS
    assert len(want) == 64 and set(seen) == want, sorted(set(seen) ^ want)


@pytest.mark.parametrize("lens,moving", [(False, False), (True, True)])
def test_adaptive_tiles_and_an_emulated_group_give_the_one_shot_frame(pkg, abi, host, torch_cuda, lens, moving):
    from test_adaptive import _tiles_match_one_shot
    torch = torch_cuda
    # an adaptive frame: every tile is the one-shot frame at the tile's own count
    sc, c1, ln = _load(host, _fog_cfg(80, 48, 32, lens, moving))
    ad, ref = _hip_scene(pkg, sc, c1, ln), _hip_scene(pkg, sc, c1, ln)
    img, n_t, _ = ad.render_adaptive(0.05, 8)
    assert ad.query("last_kernel") & MEDIUM and ad.query("last_kernel") & ACCUM
    assert len(np.unique(n_t)) > 1, np.unique(n_t)
    _tiles_match_one_shot(torch, abi, ref, img, n_t, ad.tile_grid(), what="fog adaptive")
    assert ref.query("last_kernel") & MEDIUM
    ad.close(); ref.close()
    # a 3-rank group on one device (emulated ranks: views that share the resident tables, the density table among them)
    sc, c1, ln = _load(host, _fog_cfg(40, 28, 6, lens, moving))
    gs = _hip_scene(pkg, sc, c1, ln)
    one = _one_shot(torch, gs)
    os.environ["RT_GPUS_EMULATE"] = "1"
    try:
        grp = pkg.hip.HipGroup(sc.ptr, 3, center1=c1)
    finally:
        del os.environ["RT_GPUS_EMULATE"]
    assert grp.size == 3
    if ln:
        grp.set_lens(*ln)
    for _ in range(3):
        g_rgb, g_st = grp.render_to_host()
        assert np.array_equal(g_rgb, one[0]) and g_st["segments"] == one[2]["segments"]
    grp.close(); gs.close()


def test_cli_renders_the_fog_scene_in_every_mode(pkg, host, torch_cuda, tmp_path):
    """one-shot, --passes, --denoise, --adaptive, --frames (both animation drivers) and RT_GPUS: the resident scene's frame"""
    from PIL import Image
    torch = torch_cuda
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    W, H, N = 48, 32, 6
    env0 = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    for lens, moving in ((False, False), (True, True)):
        cfg = _fog_cfg(W, H, N, lens, moving)
        tag = "lens_moving" if lens else "plain"
        p = tmp_path / f"fog_{tag}.json"
        p.write_text(json.dumps(cfg))
        sc, c1, ln = _load(host, cfg)
        gs = _hip_scene(pkg, sc, c1, ln)
        want = _one_shot(torch, gs)[0]
        assert gs.query("last_kernel") & MEDIUM
        d_want, _ = _hip_scene(pkg, sc, c1, ln).refine_to_host_denoised(N)

        def run(*a, env=env0):
            r = subprocess.run([exe, str(p), *a], capture_output=True, text=True, timeout=300, env=env)
            assert r.returncode == 0, (a, r.stderr)

        def img(name):
            return np.asarray(Image.open(tmp_path / name))
        run(str(tmp_path / f"{tag}_one.png"))
        assert np.array_equal(img(f"{tag}_one.png"), want), tag
        run(str(tmp_path / f"{tag}_passes.png"), "--passes", "3")
        assert np.array_equal(img(f"{tag}_passes.png"), want), tag
        run(str(tmp_path / f"{tag}_den.png"), "--denoise")
        assert np.array_equal(img(f"{tag}_den.png"), d_want), tag
        run(str(tmp_path / f"{tag}_ad.png"), "--adaptive", "0", "--min-spp", "2")   # (threshold 0: every tile to N)
        assert np.array_equal(img(f"{tag}_ad.png"), want), tag
        run(str(tmp_path / f"{tag}_anim"), "--frames", "2", "--orbit", "10")
        assert np.array_equal(img(f"{tag}_anim_000.png"), want), tag
        run(str(tmp_path / f"{tag}_animf"), "--frames", "2", "--orbit", "10", env=dict(env0, RT_ANIM="frames"))
        assert np.array_equal(img(f"{tag}_animf_000.png"), want) and np.array_equal(img(f"{tag}_animf_001.png"), img(f"{tag}_anim_001.png")), tag
        run(str(tmp_path / f"{tag}_g2.png"), env=dict(env0, RT_GPUS="2", RT_GPUS_EMULATE="1", RT_GATHER="peer"))
        assert np.array_equal(img(f"{tag}_g2.png"), want), tag
        # without its media the scene is another picture
        cfg0 = json.loads(json.dumps(cfg))
        cfg0["objects"] = [o for o in cfg0["objects"] if "Medium" not in o["material"]]
        p0 = tmp_path / f"clear_{tag}.json"
        p0.write_text(json.dumps(cfg0))
        r = subprocess.run([exe, str(p0), str(tmp_path / f"{tag}_clear.png")], capture_output=True, text=True, timeout=300, env=env0)
        assert r.returncode == 0 and not np.array_equal(img(f"{tag}_clear.png"), want), tag
        gs.close()
