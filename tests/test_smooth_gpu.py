"""Shading normals on triangles and meshes on the GPU, through the C ABI: small frames against the restatement
(tests/smooth_mini.py) and against the full scan bit for bit; the device form of rt_flat_normal.h through rt_hip_quad_probe (the record
object_surface<true> forms, in f64) against the host build bit for bit; three checks that need no restatement (the axis-aligned identity, the
sphere limit, set and remove); and the plumbing — updates, device input, the group, passes, shards, adaptive frames, all 64 QUADS kernels,
every refusal, the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import lane_sim
import smooth_frames as SF
import smooth_mini as SMM
import smooth_points as SP
import smooth_sim
import smooth_worlds as SW
import tri_sim
from parity import assert_parity, pooled_atol
from test_medium_gpu import _load, _one_shot, _same, _stream

QUADS, ACCUM = 512, 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
W, H, SPP = SW.W, SW.H, SW.SPP
FLAT_TABLES = ("quads", "quad_lim", "flat_bvh", "flat_bvh_order", "flat_normals")


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _scene(pkg, sc, c1=None, lens=None, quads=None, normals=None, bvh=False, library=None):
    gs = pkg.hip.HipScene(sc.ptr, 0, library=library, center1=c1, quads=quads, flat_bvh=bvh)
    if lens:
        gs.set_lens(*lens)
    if normals is not None:
        gs.set_flat_normals(normals)
    return gs


def _aovs(gs, n=SPP):
    aov = torch.zeros((gs.height, gs.width, 8), dtype=torch.float32, device="cuda:0")
    gs.render_aovs(n, aov.data_ptr(), None, _stream(torch))
    torch.cuda.synchronize()
    return aov.cpu().numpy()


def _tables(gs):
    return {name: gs.table(name) for name in FLAT_TABLES}


def _frames_equal(a, b, what):
    _same(a, b, what)
    assert a[2]["segments"] == b[2]["segments"] > 0, (what, a[2]["segments"], b[2]["segments"])


def _differs(a, b):
    return not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ------------------------------------------------------------------ frames against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("case,bvh", [(c, False) for c in SW.PARITY_CASES] + [("metal", True)])
def test_small_frames_against_the_restatement(pkg, abi, oracle, host, torch_cuda, case, bvh):
    """linear radiance, RGB8 and the exact segment identity (tests/parity.py's bar) against SmoothMini; the kernel is the one the scene
    selected without normals; "variant" 1 gives the same frame bit for bit; the AOVs are SmoothMini's in every bit"""
    sc, c1, lens, quads, normals = SF.world(host, case)
    gs = _scene(pkg, sc, c1, lens, quads, None, bvh)
    flat = _one_shot(torch, gs)
    key = gs.query("last_kernel")
    assert key & QUADS and gs.query("flat_normals") == 0 and gs.table("flat_normals") == b""
    gs.set_flat_normals(normals)
    assert gs.query("flat_normals") == len(quads) - 2 == (320 if case == "metal" else 80) and len(gs.table("flat_normals")) == 72 * len(quads) and (gs.query("flat_bvh") > 0) == bvh
    rgb, lin, st = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key
    assert _differs((rgb, lin), flat), "normals changed nothing"
    m = SF.mini_frame(oracle, abi, host, case)
    print(f"{case} bvh={bvh}: max |linear diff| {float(np.abs(lin - m['lin']).max()):.3g}, segments gpu {st['segments']} mini {m['segments']} - {m['discarded']}, fell {m['fell']}")
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(SPP))
    assert st["segments"] == m["segments"] - m["discarded"]
    if case == "glass":
        assert m["fell"][SMM.FELL_SIDE] > 0 and m["fell"][SMM.FELL_GRAZING] > 0
    gs.set_option("variant", 1)
    b = _one_shot(torch, gs)
    assert gs.query("last_kernel") == key
    _frames_equal((rgb, lin, st), b, "variant 1")
    gs.set_option("variant", 0)
    if not bvh:
        want = SF.mini(oracle, abi, sc, c1, lens, quads, normals).aovs(SPP)
        got = _aovs(gs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    gs.close()


# ------------------------------------------------------------------ the device form, bit for bit
_DEVICE_REF = {}


def _device_reference(cls):
    """the host build on a class of tests/smooth_points.py's device tables: per ray the hit decision, t, P, front (rt_flat_hit, lim = 1) and
    the normal — rt_flat_normal_shade at that P where the entry has normals; the normals as set (a refused record: none) and the records"""
    if cls not in _DEVICE_REF:
        quv, nr, rays = SP.device_table(cls)
        L, T = smooth_sim.load(), tri_sim.load()
        E, R = SP.DEVICE_ENTRIES, SP.DEVICE_REP
        with np.errstate(all="ignore"):
            kind, rec = L.prepare(nr)
            normals = np.where((kind == SMM.BAD)[:, None], 0.0, nr)
            kind, rec = L.prepare(normals)
            hit, t, P, nrm, front = np.zeros(E * R, np.int32), np.zeros(E * R), np.zeros((E * R, 3)), np.zeros((E * R, 3)), np.zeros(E * R, np.int32)
            fell = {0: 0, SMM.FELL_MM: 0, SMM.FELL_SIDE: 0, SMM.FELL_GRAZING: 0}
            for k in range(E):
                sl = slice(k * R, (k + 1) * R)
                st, hit[sl], t[sl], P[sl], nrm[sl], front[sl] = T.flat_hit_v(quv[k], 1.0, rays[sl], np.full(R, 1e300))
                assert st == 0, (cls, k)
                sel = np.flatnonzero(hit[sl] == 1) + k * R
                if kind[k] != SMM.SMOOTH or not sel.size:
                    continue
                st, nrm[sel], f = L.shade(quv[k], rec[k], rays[sel, 3:6], P[sel])
                for b in (SMM.FELL_MM, SMM.FELL_SIDE, SMM.FELL_GRAZING):
                    fell[b] += int(((f & b) != 0).sum())
                fell[0] += int((f == 0).sum())
        _DEVICE_REF[cls] = (normals, rec, hit, t, P, nrm, front, fell)
    return _DEVICE_REF[cls]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", SP.DEVICE_CLASSES)
def test_device_tables_on_the_host_build(cls):
    """the inputs of the device test, without a GPU: >= 10^5 rays per class, most of them hits, and the host build takes the fallback the
    class is about — on both sides of it"""
    normals, rec, hit, t, P, nrm, front, fell = _device_reference(cls)
    print(f"{cls}: {int(hit.sum())} of {len(hit)} rays hit; host build took {fell}")
    assert len(hit) >= 100_000 and hit.sum() > (0.2 if cls == "edges" else 0.8) * len(hit) and fell[0] > 10_000
    if cls == "opposite":
        assert fell[SMM.FELL_MM] > 10_000
    if cls == "side":
        assert fell[SMM.FELL_SIDE] > 10_000
    if cls == "grazing":
        assert fell[SMM.FELL_GRAZING] > 10_000


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", SP.DEVICE_CLASSES)
def test_device_shading_normal_equals_the_host_build(pkg, abi, torch_cuda, cls):
    """Every class of tests/smooth_points.py that can reach a shaded hit (device_table says which cannot, and why), >= 10^5 rays each: one
    scene of 1 000 triangles with their normals, each entry's 103 rays through rt_hip_quad_probe(first_quad = k, n_quads = 1) — one hit
    per thread, a launch that is no multiple of 64 — which returns the record object_surface<true> forms, i.e. what the cold function
    returned, in f64.  The accept decision, t, P and front_face are the host build's rt_flat_hit — unchanged by the normals — and the
    normal is the host build's rt_flat_normal_shade at that P, bit for bit; the resident records are the host build's"""
    from test_quad_rays_gpu import _ProbeOut, _assert_probe_equals, _dev
    from test_tri_gpu import _c_flat, _probe_scene
    quv, _, rays = SP.device_table(cls)
    normals, rec, hit, t, P, nrm, front, fell = _device_reference(cls)
    E, R = SP.DEVICE_ENTRIES, SP.DEVICE_REP
    gs = _probe_scene(pkg, abi, [_c_flat(abi, q, abi.RT_QUAD_SHAPE_TRIANGLE) for q in quv])
    try:
        gs.set_flat_normals(normals)
        assert gs.table("flat_normals") == np.ascontiguousarray(rec).tobytes()
        d_rays, d_closest = _dev(rays), _dev(np.full(E * R, 1e300))
        out = _ProbeOut(E * R)
        stream = torch.cuda.current_stream().cuda_stream
        for k in range(E):
            gs.quad_probe(d_rays.data_ptr() + 48 * k * R, d_closest.data_ptr() + 8 * k * R, R, k, 1, *out.ptrs(k * R), stream=stream)
        torch.cuda.synchronize()
        got = out.fetch()
    finally:
        gs.close()
    which = np.repeat(np.arange(E), R)
    print(f"{cls}: {int((got[0] >= 0).sum())} of {E * R} rays hit (device); host build took {fell}")
    _assert_probe_equals(cls, got, np.where(hit == 1, 1 + which, -1).astype(np.int32), t, P, nrm, front)


# ------------------------------------------------------------------ three checks that need no restatement
@pytest.mark.gpu
def test_axis_aligned_identity(pkg, abi, host, torch_cuda):
    """a box of 12 triangles, each carrying its face's axis as all three normals: m is a multiple of the axis and s exactly the axis
    (test_smooth_cpu asserts y / sqrt(y y) == 1), so the frame and the AOVs are those of ANOTHER scene, without normals, bit for bit"""
    frames = {}
    for with_normals in (True, False):
        sc, c1, lens = _load(host, SW.box_cfg(with_normals), W, H, SPP, 8, seed=5)
        n = sc.flat_normals()
        assert (n is not None) == with_normals
        gs = _scene(pkg, sc, quads=sc.quads(), normals=n)
        assert gs.query("flat_normals") == (12 if with_normals else 0)
        frames[with_normals] = (_one_shot(torch, gs), _aovs(gs))
        gs.close()
    _frames_equal(frames[True][0], frames[False][0], "axis-aligned normals")
    assert np.array_equal(frames[True][1].view(np.uint32), frames[False][1].view(np.uint32))


@pytest.mark.gpu
def test_sphere_limit(pkg, abi, oracle, host, torch_cuda):
    """a level-2 icosphere (320 faces, the scan) ON the unit sphere with normals = vertices: m = P in exact arithmetic.  Through
    rt_hip_quad_probe, in f64: the normal of every camera ray that hits the mesh is unit_vector(P) to 1e-12 per component (about 30 f64
    operations on values <= 1, |w| <= ~13 for edges ~ 0.3).  Through rt_aov_quads, one sample: the AOV normal is float(unit_vector(P))
    to one float32 ulp — the record is float32 — and the flat scene's is not"""
    from test_quad_rays_gpu import _ProbeOut, _dev
    sc, _, _ = _load(host, SW.sphere_limit_cfg(), W, H, 1, 8, seed=3)
    quads, normals = sc.quads(), sc.flat_normals()
    assert len(quads) == 320
    gs = _scene(pkg, sc, quads=quads, normals=normals, library=pkg.hip.probe_lib())
    mini = SF.mini(oracle, abi, sc, None, None, quads, normals)
    rays = np.zeros((H * W, 6))
    for y in range(H):
        for x in range(W):
            o, d = mini.begin_sample(x, y, 0)
            rays[y * W + x] = list(o) + list(d)
    out = _ProbeOut(len(rays))
    gs.quad_probe(_dev(rays).data_ptr(), _dev(np.full(len(rays), 1e300)).data_ptr(), len(rays), 0, 320, *out.ptrs(0), stream=_stream(torch))
    torch.cuda.synchronize()
    best, _, P, nrm, front = out.fetch()
    hit = best >= 0
    assert hit.sum() > 200 and (front[hit] == 1).all()
    P, nrm = P.view(np.float64)[hit], nrm.view(np.float64)[hit]
    unit = P / np.linalg.norm(P, axis=1, keepdims=True)
    worst = float(np.abs(nrm - unit).max())
    print(f"sphere limit: {int(hit.sum())} hits, max |normal - unit(P)| = {worst:.3g}")
    assert worst <= 1e-12
    aov = _aovs(gs, 1).reshape(H * W, 8)[hit]
    assert (aov[:, 7] == 1.0).all()
    f32 = unit.astype(np.float32)
    assert (np.abs(aov[:, 4:7] - f32) <= np.spacing(np.abs(f32)) ).all()
    gs.set_flat_normals(None)
    flat = _aovs(gs, 1).reshape(H * W, 8)[hit]
    assert float(np.abs(flat[:, 4:7] - f32).max()) > 1e-3
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_set_and_remove(pkg, abi, host, torch_cuda, bvh):
    """normals set and then removed: tables byte for byte and frames bit for bit those of a scene that never had any"""
    sc, c1, lens, quads, normals = SF.world(host, "metal")
    never = _scene(pkg, sc, c1, lens, quads, None, bvh)
    gs = _scene(pkg, sc, c1, lens, quads, normals, bvh)
    want_t, want_f, want_a = _tables(never), _one_shot(torch, never), _aovs(never)
    with_n = _one_shot(torch, gs)
    assert _differs(with_n, want_f) and gs.table("quads") == want_t["quads"] and gs.table("flat_bvh") == want_t["flat_bvh"]
    gs.set_flat_normals(None)
    assert gs.query("flat_normals") == 0 and _tables(gs) == want_t
    _frames_equal(_one_shot(torch, gs), want_f, "removed")
    assert np.array_equal(_aovs(gs).view(np.uint32), want_a.view(np.uint32))
    gs.set_flat_normals(np.zeros((len(quads), 9)))          # nine zeros everywhere: no entry has normals, no table
    assert gs.query("flat_normals") == 0 and _tables(gs) == want_t
    gs.set_flat_normals(normals)                            # ... and back
    _frames_equal(_one_shot(torch, gs), with_n, "set again")
    gs.close(); never.close()


# ------------------------------------------------------------------ plumbing
def _moved(quads, normals):
    """the geometry turned a little about the y axis and lifted, with the normals turned alike"""
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    quv = np.array([list(q.q) + list(q.u) + list(q.v) for q in quads]).reshape(-1, 3, 3)
    out = quv @ R.T
    out[:, 0, 1] += 0.15
    return out.reshape(-1, 9), (normals.reshape(-1, 3, 3) @ R.T).reshape(-1, 9)


def _with_geometry(quads, quv):
    out = (type(quads[0]) * len(quads))(*quads)
    for k in range(len(out)):
        out[k].q[:], out[k].u[:], out[k].v[:] = quv[k, 0:3], quv[k, 3:6], quv[k, 6:9]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["scan", "refit", "rebuild"])
def test_update_flats_then_normals_equals_a_fresh_scene(pkg, abi, host, torch_cuda, route):
    sc, c1, lens, quads, normals = SF.world(host, "metal")
    quv1, n1 = _moved(quads, normals)
    bvh = route != "scan"
    gs = _scene(pkg, sc, c1, lens, quads, normals, bvh)
    before = _one_shot(torch, gs)
    gs.update_flats(quv1, rebuild=route == "rebuild")
    assert gs.query("flat_normals") == len(quads) - 2 and gs.table("flat_normals") == np.ascontiguousarray(smooth_sim.load().prepare(normals)[1]).tobytes()   # kept as set
    stale = _one_shot(torch, gs)
    gs.set_flat_normals(n1)
    fresh = _scene(pkg, sc, c1, lens, _with_geometry(quads, quv1), n1, bvh)
    got, want = _one_shot(torch, gs), _one_shot(torch, fresh)
    names = FLAT_TABLES if route != "refit" else ("quads", "quad_lim", "flat_normals")    # (a refit keeps the order table and the tree it had)
    a, b = _tables(gs), _tables(fresh)
    for name in names:
        assert a[name] == b[name], (route, name)
    _frames_equal(got, want, route)
    assert _differs(got, before) and _differs(got, stale)
    gs.update_spheres([list(s.center) for s in sc.c.spheres[:sc.c.n_spheres]])     # the spheres where they are: the normals stay
    assert gs.table("flat_normals") == b["flat_normals"]
    _frames_equal(_one_shot(torch, gs), want, route + ", after update_spheres")
    gs.close(); fresh.close()


@pytest.mark.gpu
def test_device_input_builds_the_host_paths_table(pkg, abi, host, torch_cuda):
    sc, c1, lens, quads, normals = SF.world(host, "glass")
    a, b = _scene(pkg, sc, c1, lens, quads, normals), _scene(pkg, sc, c1, lens, quads)
    b.set_flat_normals(torch.from_numpy(normals).to("cuda:0"))
    assert a.table("flat_normals") == b.table("flat_normals") == np.ascontiguousarray(smooth_sim.load().prepare(normals)[1]).tobytes()
    _frames_equal(_one_shot(torch, a), _one_shot(torch, b), "device input")
    b.set_flat_normals(torch.from_numpy(normals).to("cuda:0").t().contiguous().t())     # not contiguous: through the host
    assert a.table("flat_normals") == b.table("flat_normals")
    a.close(); b.close()


@pytest.mark.gpu
def test_group_of_two_equals_one_rank(pkg, abi, host, torch_cuda, monkeypatch):
    sc, c1, lens, quads, normals = SF.world(host, "metal")
    one = _scene(pkg, sc, c1, lens, quads, normals)
    want = _one_shot(torch, one)
    monkeypatch.setenv("RT_GPUS_EMULATE", "1")
    grp = pkg.hip.HipGroup(sc.ptr, 2, quads=quads)
    monkeypatch.delenv("RT_GPUS_EMULATE")
    try:
        assert grp.size == 2
        flat, _ = grp.render_to_host()
        assert not np.array_equal(flat, want[0])
        bad = normals.copy(); bad[7, 4] = np.inf
        with pytest.raises(pkg.host.RtError) as e:
            grp.set_flat_normals(bad)
        assert "quad 7: normal" in str(e.value) and np.array_equal(grp.render_to_host()[0], flat)
        grp.set_flat_normals(normals)
        frames = [np.zeros((H, W, 3), np.uint8) for _ in range(2)]
        grp.submit(frames[0]); grp.submit(frames[1])       # (the second one renders through the ranks' views)
        stats = [grp.collect(), grp.collect()]
        for f, st in zip(frames, stats):
            assert np.array_equal(f, want[0]) and st["segments"] == want[2]["segments"]
        grp.set_flat_normals(None, len(quads))
        assert np.array_equal(grp.render_to_host()[0], flat)
    finally:
        grp.close(); one.close()


@pytest.mark.gpu
def test_composition_is_the_one_shot_frame(pkg, abi, host, torch_cuda):
    """passes (0, 1), (1, 3), (3, 4), row shards {8, r, 3} and rt_hip_render_adaptive_to_host at threshold 0: each the one-shot frame"""
    sc, c1, lens, quads, normals = SF.world(host, "glass")
    gs = _scene(pkg, sc, c1, lens, quads, normals)
    one = _one_shot(torch, gs)
    acc = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda:0")
    segs = 0
    for b, e in ((0, 1), (1, 3), (3, 4)):
        gs.accumulate(acc.data_ptr(), b, e - b, None, _stream(torch))
        segs += gs.wait()["segments"]
        assert gs.query("last_kernel") & QUADS and gs.query("last_kernel") & ACCUM
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    gs.resolve(acc.data_ptr(), SPP, rgb.data_ptr(), lin.data_ptr(), None, _stream(torch))
    torch.cuda.current_stream().synchronize()
    _same(one, (rgb.cpu().numpy(), lin.cpu().numpy()), "passes")
    assert segs == one[2]["segments"]
    frame_rgb, frame_lin, segs = np.zeros_like(one[0]), np.zeros_like(one[1]), 0
    for r in range(3):
        t = abi.RtRowTiles(8, r, 3)
        rows = abi.tiles_global_rows(H, t)
        s_rgb, s_lin, st = _one_shot(torch, gs, t, len(rows))
        frame_rgb[rows], frame_lin[rows] = s_rgb, s_lin
        segs += st["segments"]
    _same(one, (frame_rgb, frame_lin), "row shards")
    assert segs == one[2]["segments"]
    ad_rgb, ad_spp, _ = gs.render_adaptive(0.0, 2)
    assert (ad_spp == SPP).all() and np.array_equal(ad_rgb, one[0])
    gs.close()


@pytest.mark.gpu
def test_denoise_and_temporal_surface_stay_finite(pkg, abi, host, torch_cuda):
    sc, c1, lens, quads, normals = SF.world(host, "metal")
    gs = _scene(pkg, sc, c1, lens, quads, normals)
    out, st = gs.refine_to_host_denoised(SPP)
    assert out.any() and st["segments"] > 0
    gs.temporal_surface(True)
    a, _ = gs.render_frame_temporal_to_host(0)
    b, _ = gs.render_frame_temporal_to_host(1)
    hist = gs.temporal_history()
    assert a.any() and b.any() and np.isfinite(hist).all()
    assert np.isfinite(_aovs(gs)).all()
    gs.close()


@pytest.mark.gpu
def test_all_64_quads_kernels_run_with_normals(pkg, abi, host, torch_cuda):
    """the 32 mesh cells of tests/test_feature_matrix.py, one-shot and accumulating: each reports its key, unchanged by the normals, the
    frame differs from the flat one, and the grid walk equals the full scan bit for bit"""
    import test_feature_matrix as FM
    seen = set()
    for s in FM.MESH:
        key = FM._key(s)
        sc, c1, lens, quads = FM._world(host, s)
        tri = np.array([q.reserved == abi.RT_QUAD_SHAPE_TRIANGLE for q in quads])
        assert tri.sum() == FM.N_MESH_TRIS
        geo = np.array([[list(q.u), list(q.v)] for q in quads])
        N = np.cross(geo[:, 0], geo[:, 1]); N /= np.linalg.norm(N, axis=1, keepdims=True)
        t = geo[:, 0] / np.linalg.norm(geo[:, 0], axis=1, keepdims=True)
        normals = np.where(tri[:, None], np.concatenate([N + 0.8 * t, N - 0.8 * t, N], axis=1), 0.0)
        gs = _scene(pkg, sc, c1, lens, quads)
        flat = _one_shot(torch, gs)
        gs.set_flat_normals(normals)
        assert gs.query("flat_normals") == FM.N_MESH_TRIS
        one = FM._frame_and_passes(torch, gs, key, FM._id(s))          # (asserts last_kernel == key, then key | ACCUM, frames equal)
        seen |= {key, key | ACCUM}
        assert _differs(one, flat), FM._id(s)
        gs.set_option("variant", 1)
        _frames_equal(_one_shot(torch, gs), one, FM._id(s) + ": variant 1")
        gs.close()
    assert len(seen) == 64 and all(k & QUADS for k in seen)


@pytest.mark.gpu
def test_headline_scene_keeps_its_kernel(pkg, load_scene, torch_cuda):
    sc = load_scene("cover", 48, 32, 2)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    _one_shot(torch, gs)
    assert gs.query("last_kernel") == 3 and gs.query("flat_normals") == 0 and gs.table("flat_normals") == b""
    with pytest.raises(pkg.host.RtError):
        gs.set_flat_normals(np.zeros((1, 9)))              # no flat primitive
    gs.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(pkg, abi, host, torch_cuda):
    sc, c1, lens, quads, normals = SF.world(host, "metal")       # entries 0 and 1 are the floor's and the wall's parallelograms
    assert quads[0].reserved == abi.RT_QUAD_SHAPE_PARALLELOGRAM and quads[2].reserved == abi.RT_QUAD_SHAPE_TRIANGLE
    L = pkg.hip.lib()
    for bvh in (False, True):
        gs = _scene(pkg, sc, c1, lens, quads, normals, bvh)
        before, tables = _one_shot(torch, gs), _tables(gs)

        def refused(needle, arr=None, n=None, flags=0, ptr=None):
            arr = np.ascontiguousarray(arr if arr is not None else normals)
            with pytest.raises(pkg.host.RtError) as e:
                pkg.hip._check(L.rt_hip_scene_set_flat_normals(gs._h, arr.ctypes.data if ptr is None else ptr, len(arr) if n is None else n, flags), L)
            assert e.value.code == abi.RT_ERR_INVALID and needle in str(e.value), str(e.value)
            assert _tables(gs) == tables
            _frames_equal(_one_shot(torch, gs), before, needle)
        bad = normals.copy(); bad[40, 3] = np.nan; bad[60, 0:3] = 0.0
        refused("quad 40: normal", bad)
        bad = normals.copy(); bad[60, 0:3] = 0.0; bad[70, 8] = np.inf
        refused("quad 60: normal", bad)
        bad = normals.copy(); bad[5, 6:9] = 1e-170
        refused("quad 5: normal", bad)
        bad = normals.copy(); bad[1, 2] = 1.0; bad[9, 0] = np.nan
        refused("quad 1: normal", bad)                         # a parallelogram with normals, the lowest bad entry
        refused("n_quads", normals[:-1])
        refused("unknown flag", flags=4)
        refused("unknown flag", flags=abi.RT_UPDATE_FLATS_REBUILD)
        gs.close()
    with pytest.raises(pkg.host.RtError):
        pkg.hip._check(L.rt_hip_scene_set_flat_normals(None, None, 0, 0), L)


@pytest.mark.gpu
def test_rays_probe_first_hits_are_unchanged_by_normals(pkg, abi, host, torch_cuda):
    """four frames (64 x 48, spp 2) through rt_hip_render_rays_probe: (closest, best) of every camera ray with normals are those without,
    and the host build's bit for bit"""
    from test_quad_rays_gpu import _dev
    for case, bvh in (("metal", False), ("metal", True), ("glass", False), ("checker", True)):
        sc, c1, lens = _load(host, SW.parity_cfg(case), 64, 48, 2, 8, seed=13)
        quads, normals = sc.quads(), sc.flat_normals()
        rng = np.random.default_rng(77)
        rays = np.concatenate([np.tile([0.0, 1.0, 6.0], (64 * 48, 1)), rng.uniform(-1, 1, (64 * 48, 3)) * [0.5, 0.35, 0.0] + [-0.08, -0.05, -1.0]], axis=1)
        d_rays = _dev(rays)
        rec = {}
        for with_n in (False, True):
            gs = _scene(pkg, sc, c1, None, quads, normals if with_n else None, bvh, library=pkg.hip.probe_lib())
            t = torch.zeros(64 * 48, dtype=torch.float64, device="cuda:0")
            best = torch.full((64 * 48,), -7, dtype=torch.int32, device="cuda:0")
            rgb = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda:0")
            gs.render_rays_probe(d_rays.data_ptr(), rgb.data_ptr(), 0, t.data_ptr(), best.data_ptr())
            rec[with_n] = (t.cpu().numpy().view(np.uint64), best.cpu().numpy(), rgb.cpu().numpy())
            gs.close()
        assert np.array_equal(rec[True][0], rec[False][0]) and np.array_equal(rec[True][1], rec[False][1]), (case, bvh)
        # ... and the host build's (tests/lanesim/ hit_world over the same tables, no contraction): the megakernel's own copy of the flat test
        rc, h_best, h_t, _ = lane_sim.load(abi).hit_world_v(sc.c, rays, quads=quads)
        assert rc == 0 and np.array_equal(rec[True][1], h_best), (case, bvh, int((rec[True][1] != h_best).sum()))
        hit = h_best >= 0
        assert np.array_equal(rec[True][0][hit], h_t.view(np.uint64)[hit]), (case, bvh, int((rec[True][0][hit] != h_t.view(np.uint64)[hit]).sum()))
        n_sph = sc.c.n_spheres
        assert (rec[True][1] >= n_sph + 2).sum() > 100, (case, bvh)        # rays that meet the mesh first
        assert not np.array_equal(rec[True][2], rec[False][2]), (case, bvh)


# ------------------------------------------------------------------ the CLI
@pytest.mark.gpu
def test_cli_renders_the_example_with_its_normals(pkg, abi, host, torch_cuda, tmp_path):
    """a 48 x 32 cut of scenes/make_smooth_scene.py (both icospheres at subdivision 2) through `raytracer`: the API frame of the same file,
    and NOT the frame of the file with "normals" stripped"""
    from PIL import Image
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_smooth_scene", os.path.join(ROOT, "scenes", "make_smooth_scene.py"))
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scenes"))
    try:
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scenes"))
    cfg = json.loads(mod.make(2))
    cfg.update(width=W, height=H, samples_per_pixel=SPP, max_depth=8)
    assert sum("normals" in o.get("mesh", {}) for o in cfg["objects"]) == 2
    env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
    imgs = {}
    for name, c in (("smooth", cfg), ("flat", SW.strip_normals(cfg))):
        (tmp_path / f"{name}.json").write_text(json.dumps(c))
        r = subprocess.run([EXE, str(tmp_path / f"{name}.json"), str(tmp_path / f"{name}.png")], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.stdout, r.stderr)
        imgs[name] = np.asarray(Image.open(tmp_path / f"{name}.png").convert("RGB"))
    assert not np.array_equal(imgs["smooth"], imgs["flat"]), "the CLI ignored the file's normals"
    sc = host.Scene.load(str(tmp_path / "smooth.json"))
    assert sc.flat_bvh() and sc.flat_normals() is not None
    gs = _scene(pkg, sc, quads=sc.quads(), normals=sc.flat_normals(), bvh=True)
    api, _ = gs.render_to_host()
    gs.close()
    assert np.array_equal(api, imgs["smooth"])
