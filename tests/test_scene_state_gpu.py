"""What a resident scene caches between calls, and which event drops which cache (the table at RtHipScene in csrc/hip/rt_hip_api.hip):
the host forms' progressive accumulator with its cached AOV record, the rounds of the last adaptive frame, the temporal history.
One tiny scene; every case brings all three to a known state, applies ONE event, and asks the scene what it still holds."""
import json

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded, as collecting the whole suite does: the process then holds ONE HIP runtime, torch's)
    import torch  # noqa: F401
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 24, 16, 4, 8
LOOK_FROM, LOOK_AT, VUP, VFOV = (6.0, 1.5, 3.0), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 35.0
# a ground sphere and seven small ones: Lambertian, Metal and Glass
SMALL = [((0.0, 0.5, 0.0), 0.5, {"Glass": {"index_of_refraction": 1.5}}),
         ((-1.2, 0.4, 0.6), 0.4, {"Lambertian": {"albedo": [0.7, 0.2, 0.2]}}),
         ((1.1, 0.4, -0.7), 0.4, {"Metal": {"albedo": [0.8, 0.7, 0.6], "fuzz": 0.1}}),
         ((0.6, 0.3, 1.2), 0.3, {"Lambertian": {"albedo": [0.2, 0.6, 0.3]}}),
         ((-0.5, 0.3, -1.4), 0.3, {"Metal": {"albedo": [0.6, 0.6, 0.9], "fuzz": 0.0}}),
         ((1.9, 0.3, 0.9), 0.3, {"Glass": {"index_of_refraction": 1.3}}),
         ((-2.0, 0.35, -0.3), 0.35, {"Lambertian": {"albedo": [0.3, 0.3, 0.8]}})]
CENTRES = np.array([(0.0, -100.0, 0.0)] + [c for c, _, _ in SMALL], np.float64)
MOVED = CENTRES + np.array([(0.0, 0.0, 0.0)] + [(0.3 * (-1) ** i, 0.05 * i, -0.2) for i in range(len(SMALL))])
# the update_flats case alone adds a flat primitive: a red parallelogram just above the ground, between the spheres and the camera (q, u, v)
QUV = np.array([[2.2, 0.05, 1.2, 0.0, 0.0, 1.0, 1.2, 0.0, 0.0]], np.float64)
QUV_MOVED = QUV + np.array([[-0.4, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])


def _text(centres=CENTRES):
    radii = [100.0] + [r for _, r, _ in SMALL]
    mats = [{"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}] + [m for _, _, m in SMALL]
    objs = [{"center": dict(zip("xyz", (float(v) for v in c))), "radius": r, "material": m} for c, r, m in zip(centres, radii, mats)]
    return json.dumps({"width": W, "height": H, "samples_per_pixel": SPP, "max_depth": DEPTH, "sky": {"texture": ""},
                       "camera": {"look_from": dict(zip("xyz", LOOK_FROM)), "look_at": dict(zip("xyz", LOOK_AT)), "vup": dict(zip("xyz", VUP)),
                                  "vfov": VFOV, "aspect": W / H}, "objects": objs})


def _quad(abi, quv):
    """QUV or QUV_MOVED as the one Lambertian abi.RtQuad a scene is created with"""
    q = abi.RtQuad(kind=abi.RT_MAT_LAMBERTIAN, reserved=abi.RT_QUAD_SHAPE_PARALLELOGRAM)
    q.q[:], q.u[:], q.v[:] = quv[0, 0:3], quv[0, 3:6], quv[0, 6:9]
    q.albedo[:] = [0.9, 0.1, 0.1]
    return [q]


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _same_camera(host, gs, sc):
    gs.set_camera(list(sc.c.cam_origin), list(sc.c.cam_lower_left), list(sc.c.cam_horizontal), list(sc.c.cam_vertical))


def _other_camera(host, gs, sc):
    d = host.camera_derive([5.0, 2.0, 4.0], list(LOOK_AT), list(VUP), VFOV, W / H)
    gs.set_camera(d["origin"], d["lower_left_corner"], d["horizontal"], d["vertical"])


def _lens(host, radius):
    d = host.camera_derive_lens(list(LOOK_FROM), list(LOOK_AT), list(VUP), VFOV, W / H, 0.2, 1.0)
    return d["u"], d["v"], radius


def _option(key, value):
    return lambda host, gs, sc: gs.set_option(key, value)


def _new_order_key(host, gs, sc):
    gs.set_option("tile_log2", 1)   # (itself an "other option"; the frame behind it is a launch of another tile geometry)
    gs.render_to_host()


KEPT, DROPPED = True, False
# event: (what it does, accumulator, adaptive rounds, temporal history)
EVENTS = {
    "camera_same": (_same_camera, DROPPED, KEPT, KEPT),
    "camera_other": (_other_camera, DROPPED, KEPT, KEPT),
    "lens_same": (lambda host, gs, sc: gs.set_lens(*_lens(host, 0.0)), KEPT, KEPT, KEPT),    # (pinhole to pinhole)
    "lens_other": (lambda host, gs, sc: gs.set_lens(*_lens(host, 0.1)), DROPPED, KEPT, KEPT),
    "option_tile_order": (_option("tile_order", 1), KEPT, KEPT, KEPT),
    "option_tile_affinity": (_option("tile_affinity", 2), KEPT, KEPT, KEPT),
    "option_seed": (_option("seed", 12345), DROPPED, KEPT, KEPT),
    "option_max_depth": (_option("max_depth", 5), DROPPED, KEPT, KEPT),
    "option_accum_reset": (_option("accum_reset", 1), DROPPED, KEPT, KEPT),
    "option_samples_per_pixel": (_option("samples_per_pixel", 6), KEPT, KEPT, KEPT),
    "option_variant": (_option("variant", 1), KEPT, KEPT, KEPT),
    "option_tile_log2": (_option("tile_log2", 1), KEPT, KEPT, KEPT),
    "option_tile_shape": (_option("tile_shape", 1), KEPT, KEPT, KEPT),
    "option_chunk_spp": (_option("chunk_spp", 2), KEPT, KEPT, KEPT),
    "option_tile_batch": (_option("tile_batch", 1), KEPT, KEPT, KEPT),
    "option_light_nest_pool": (_option("light_nest_pool", 0), KEPT, KEPT, KEPT),
    "update_spheres": (lambda host, gs, sc: gs.update_spheres(MOVED), DROPPED, DROPPED, KEPT),
    "update_flats": (lambda host, gs, sc: gs.update_flats(QUV_MOVED), DROPPED, DROPPED, DROPPED),    # (its scene alone has a quad)
    "new_order_key": (_new_order_key, KEPT, KEPT, KEPT),
    "temporal_surface_on": (lambda host, gs, sc: gs.temporal_surface(True), KEPT, KEPT, DROPPED),
    "temporal_surface_unchanged": (lambda host, gs, sc: gs.temporal_surface(False, 0.5), KEPT, KEPT, KEPT),
    "temporal_reset": (lambda host, gs, sc: gs.temporal_reset(), KEPT, KEPT, DROPPED),
}


def _fill(gs):
    """every cache of the scene in a known state: 4 samples in the accumulator with the AOV record of its start cached (the second pass is
    the denoised form, which is what computes the record), the rounds of one adaptive frame, a temporal history of two frames"""
    gs.refine_to_host(2)
    gs.refine_to_host_denoised(2)
    assert gs.query("accum_samples") == 4
    gs.render_adaptive(0.0, 2)     # (threshold 0: every tile goes on from 2 to 4 samples, two rounds)
    rounds = gs.adaptive_rounds()
    assert [(t, n) for t, n, _ in rounds] == [(rounds[0][0], 2), (rounds[0][0], 4)] and rounds[0][0] > 1, rounds
    gs.render_frame_temporal_to_host(0)
    gs.render_frame_temporal_to_host(1)
    assert gs.temporal_history()[..., 3].max() > 1.0     # (the second frame found the first one's history)
    assert gs.query("accum_samples") == 4 and gs.adaptive_rounds() == rounds     # (the three states do not touch each other)
    return rounds


@pytest.mark.parametrize("event", list(EVENTS))
def test_an_event_drops_the_caches_its_row_names_and_no_other(pkg, host, abi, torch_cuda, event):
    apply, accum, adaptive, history = EVENTS[event]
    sc = host.Scene.loads(_text())
    gs = pkg.hip.HipScene(sc.ptr, 0, quads=_quad(abi, QUV) if event == "update_flats" else None)
    ref = None
    try:
        before = gs.render_to_host()[0]
        rounds = _fill(gs)
        apply(host, gs, sc)
        assert gs.query("accum_samples") == (4 if accum is KEPT else 0), event
        assert gs.adaptive_rounds() == (rounds if adaptive is KEPT else []), event
        if history is KEPT:
            assert gs.temporal_history().shape == (H, W, 4)
        else:
            with pytest.raises(pkg.host.RtError) as e:
                gs.temporal_history()
            assert e.value.code == abi.RT_ERR_INVALID, (event, e.value)
        if event in ("camera_other", "lens_other"):
            # the next denoised pass is that of a scene that never saw the old view: no AOV record of it survived
            ref = pkg.hip.HipScene(sc.ptr, 0)
            apply(host, ref, sc)
            got, want = gs.refine_to_host_denoised(2)[0], ref.refine_to_host_denoised(2)[0]
            assert np.array_equal(got, want), (event, int((got != want).sum()))
            assert gs.query("accum_samples") == 2
        if event == "update_spheres":
            # (tests/test_update_gpu.py compares tables, counters and walks at its own sizes; here: the frame behind the dropped state)
            keep = host.Scene.loads(_text(MOVED))
            ref = pkg.hip.HipScene(keep.ptr, 0)
            got, want = gs.render_to_host()[0], ref.render_to_host()[0]
            assert np.array_equal(got, want), int((got != want).sum())
            assert not np.array_equal(want, before)     # (the spheres did move in the picture)
            got, want = gs.refine_to_host_denoised(2)[0], ref.refine_to_host_denoised(2)[0]
            assert np.array_equal(got, want), int((got != want).sum())
        if event == "update_flats":
            # (tests/test_flat_update_gpu.py compares records and frames at its own sizes; here: the frame behind the dropped state)
            ref = pkg.hip.HipScene(sc.ptr, 0, quads=_quad(abi, QUV_MOVED))
            got, want = gs.render_to_host()[0], ref.render_to_host()[0]
            assert np.array_equal(got, want), int((got != want).sum())
            assert not np.array_equal(want, before)     # (the quad did move in the picture)
    finally:
        gs.close()
        if ref is not None:
            ref.close()


def test_the_tiny_scene_is_the_shape_the_cases_need(pkg, host, torch_cuda):
    """more than one pixel tile, paths that bounce off a sphere and paths that leave for the sky before the depth limit"""
    sc = host.Scene.loads(_text())
    gs = pkg.hip.HipScene(sc.ptr, 0)
    try:
        _, _, tx, ty = gs.tile_grid()
        assert tx * ty > 1
        frame, st = gs.render_to_host()
        assert st["samples"] == W * H * SPP and W * H * SPP < st["segments"] < W * H * SPP * DEPTH
        assert frame.std() > 0
    finally:
        gs.close()
