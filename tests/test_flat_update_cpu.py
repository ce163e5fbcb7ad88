"""Moving the flat primitives of a resident scene, without a GPU: the device code of rt_flat_build.hip compiled by g++ against
the kernel-language emulation (tests/update/emu + tests/flatupdate/emu) against the host's rt_quad_prepare, flat_entry_box and a plain
refit, byte for byte; the host builder after flat_entry_box moved into the shared header against digests recorded before the move; the
conditions the GPU tests put on their scenes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import flat_bvh_sim as F
import flat_update_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "flat_update_host_digest.json")
W, H = 48, 32
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


def _sim(abi):
    return F.load(abi)


# ------------------------------------------------------------------ the host builder builds what it built
def _digest_worlds():
    from test_flat_bvh_cpu import _world
    out = {name: (U.world(name), 1) for name in ("2048", "1025")}
    out["2048 rippled"] = (U.moved(U.world("2048"), "ripple", 2), 1)
    out["outliers 1025"] = _world("outliers", 1025)
    out["generic 4096"] = _world("generic", 4096)
    return out


def host_build_digests(abi):
    """{world: sha256 over the node table and the order table} of build_tables + build_flat_bvh on the worlds above"""
    from test_flat_bvh_gpu import _c_scene
    sim = _sim(abi)
    out = {}
    for name, (quv, shapes) in _digest_worlds().items():
        sc, keep = _c_scene(abi, W, H)
        nodes, order = sim.scene_tables(sc, F.flats_array(abi, quv, shapes))
        out[name] = U.digest(nodes, order)
    return out


def test_host_builder_builds_the_bytes_it_built_before_the_move(abi):
    """flat_entry_box is now the shared RT_HD function of rt_flat_build.h (plain comparisons instead of std::min / std::max): the node and
    order tables of five worlds, one of them with refused entries, against digests recorded from the builder before the move"""
    want = json.load(open(GOLDEN))
    got = host_build_digests(abi)
    assert got == want
    assert len(set(got.values())) == len(got)
    # (and the builder's box is the shared function's: rt_tables.h no longer has one of its own)
    hip_dir = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "hip")
    assert "bool flat_entry_box(" not in open(os.path.join(hip_dir, "rt_tables.h")).read()
    assert "RT_HD bool flat_entry_box(" in open(os.path.join(hip_dir, "rt_flat_build.h")).read()


# ------------------------------------------------------------------ the device code, emulated
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """csrc/hip/rt_flat_build.hip compiled by g++ against the emulation (real threads per workgroup, a barrier, host atomics), behind the C
    interface of tests/flatupdate/flat_update_emu.cpp"""
    hip_dir = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "hip")
    hdr = open(os.path.join(hip_dir, "rt_flat_build.h")).read()
    decl = hdr[hdr.index("#if defined(__HIPCC__)"):].replace("#if defined(__HIPCC__)", "").replace("#include <hip/hip_runtime.h>", "").rsplit("#endif", 1)[0]
    body = open(os.path.join(hip_dir, "rt_flat_build.hip")).read().replace("#include <hip/hip_runtime.h>", "").replace('#include "rt_flat_build.h"', "")
    d = tmp_path_factory.mktemp("flat_update_emu")
    src = d / "emu.cpp"
    src.write_text('#include "hip/hip_runtime.h"\n#include "' + os.path.join(hip_dir, "rt_tables.h") + '"\n' + decl + body
                   + open(os.path.join(ROOT, "tests", "flatupdate", "flat_update_emu.cpp")).read())
    so = d / "libflat_update_emu.so"
    subprocess.run(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-DRT_TEST_PROBES", "-Wno-unknown-pragmas",
                    "-I", os.path.join(ROOT, "tests", "flatupdate", "emu"), str(src), "-o", str(so), "-lpthread"], check=True)
    L = C.CDLL(str(so))
    P, u32 = C.c_void_p, C.c_uint32
    L.fu_update.argtypes = [P, P, u32, P, u32, P, u32, P, P, P, P]
    L.fu_host_records.argtypes = [P, u32, P, P]
    L.fu_host_records.restype = None
    return L


def _lim(shapes, n):
    shapes = np.broadcast_to(np.asarray(shapes), (n,))
    return np.where(shapes == 1, 1.0, 2.0) if (shapes == 1).any() else None


def _emulated_update(emu, sim, abi, old, new, shapes, structure=True):
    """one update old -> new -> (records bytes, node bytes, status, shape, the live structure)"""
    n = len(old)
    new = np.ascontiguousarray(new, np.float64)
    lim = _lim(shapes, n)
    nodes, order, n_always = sim.build(F.flats_array(abi, old, shapes)) if structure else (np.zeros(0, F.NODE), np.zeros(n, np.uint32), 0)
    rec = np.full((n, 128), 0xAB, np.uint8)
    out_nodes = np.full((len(nodes), 64), 0xCD, np.uint8)
    status, shape = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    assert emu.fu_update(new.ctypes.data, None if lim is None else lim.ctypes.data, n, nodes.ctypes.data if structure else None, len(nodes), order.ctypes.data,
                         n_always, rec.ctypes.data, out_nodes.ctypes.data, status.ctypes.data, shape.ctypes.data) == 0
    return rec, out_nodes.tobytes(), status.tolist(), shape.tolist(), (nodes, order, n_always)


def _host_records(emu, quv):
    quv = np.ascontiguousarray(quv, np.float64)
    rec, bad = np.full((len(quv), 128), 0xAB, np.uint8), np.zeros(len(quv), np.int32)
    emu.fu_host_records(quv.ctypes.data, len(quv), rec.ctypes.data, bad.ctypes.data)
    return rec, bad


def _mixed37():
    from quad_rays import _quads
    rng = np.random.default_rng(37)
    return _quads(rng, 37), rng.integers(0, 2, 37)


def _emu_worlds():
    """name -> (old rows, new rows, shapes): 37 mixed entries; the heightfield under the three moves; a world with refused entries whose
    refused set stays"""
    from test_flat_bvh_cpu import _world
    quv, shapes = _mixed37()
    out = {"mixed37": (quv, quv * np.float64(1.25) + np.float64(0.375), shapes)}
    for mv in U.MOVES:
        out["2048 " + mv] = (U.world("2048"), U.moved(U.world("2048"), mv), 1)
    ov, os_ = _world("outliers", 133)
    moved = ov.copy()
    moved[:, :3] += [0.5, -0.25, 0.125]
    out["outliers133"] = (ov, moved, os_)
    return out


@pytest.mark.parametrize("name", ["mixed37", "2048 translate", "2048 ripple", "2048 scramble", "outliers133"])
def test_emulated_device_update_equals_the_host(emu, abi, name):
    """records: rt_quad_prepare's bytes; nodes: order and topology as they were, every box the min / max over flat_entry_box of the entries
    of the node's subtree (the plain host refit), always-visited leaves infinite; the status block clean"""
    sim = _sim(abi)
    old, new, shapes = _emu_worlds()[name]
    rec, nodes_b, status, shape, (nodes, order, n_always) = _emulated_update(emu, sim, abi, old, new, shapes)
    want_rec, bad = _host_records(emu, new)
    assert not bad.any() and rec.tobytes() == want_rec.tobytes()
    assert status == [NONE, NONE, 0, 0], status
    flats_new = F.flats_array(abi, new, shapes)
    want = U.refit_nodes(sim, flats_new, nodes, order)
    assert nodes_b == want.tobytes()
    got = np.frombuffer(nodes_b, F.NODE)
    assert sim.check(got, order, len(old)) == ""
    assert (n_always > 0) == (name == "outliers133") and shape[3] == (n_always + 3) // 4
    assert np.isinf(got["lo"][:shape[3]]).all() and np.isfinite(got["lo"][shape[3]:]).all()
    assert (nodes["count"] == 0).any() and shape[0] >= 1 and shape[1] == shape[0]          # inner nodes; one launch per height, none empty
    assert shape[0] <= 2 * int(np.ceil(np.log2(len(old))))
    assert nodes_b != nodes.tobytes()                                                        # (the move moved boxes)
    # the same entries through a scene without the structure: the records alone
    rec2, none, status2, _, _ = _emulated_update(emu, sim, abi, old, new, shapes, structure=False)
    assert rec2.tobytes() == want_rec.tobytes() and none == b"" and status2 == [NONE, NONE, 0, 0]


def test_emulated_refit_to_the_geometry_of_the_build_restores_the_built_nodes(emu, abi):
    """the builder's own table comes back byte for byte: a refit is as exact as a build"""
    sim = _sim(abi)
    for old, shapes in ((U.world("2048"), 1), _mixed37()):
        _, nodes_b, status, _, (nodes, order, _) = _emulated_update(emu, sim, abi, old, old, shapes)
        assert nodes_b == nodes.tobytes() and status == [NONE, NONE, 0, 0]


def test_emulated_status_block(emu, abi):
    """the lowest bad index of each class; a refused-set change in either direction asks for a rebuild"""
    sim = _sim(abi)
    old, shapes = _mixed37()
    new = old.copy()
    new[30, 4], new[12, 0] = np.inf, np.nan
    assert _emulated_update(emu, sim, abi, old, new, shapes)[2] == [12, NONE, 0, 0]
    new = old.copy()
    new[20, 6:9] = new[20, 3:6]            # v = u: cross(u, v) = 0
    new[7, 3:6] = 0.0
    new[33, 1] = -np.inf
    assert _emulated_update(emu, sim, abi, old, new, shapes)[2] == [33, 7, 0, 0]
    thin = U.needle(old, 5)
    assert _emulated_update(emu, sim, abi, old, thin, shapes)[2] == [NONE, NONE, 1, 0]
    assert _emulated_update(emu, sim, abi, thin, old, shapes)[2] == [NONE, NONE, 1, 0]
    far = old.copy()
    far[9, 0] = 2.0 ** 41                  # a corner crossed 2^40
    far[11, 0] = -2.0 ** 41
    assert _emulated_update(emu, sim, abi, old, far, shapes)[2] == [NONE, NONE, 2, 0]
    assert _emulated_update(emu, sim, abi, thin, thin * [1, 1, 1, 2, 1, 1, 1, 1, 1], shapes)[2] == [NONE, NONE, 0, 0]   # (still a needle: no change)


# ------------------------------------------------------------------ the conditions on the GPU tests' scenes, on the host build
@pytest.mark.parametrize("name", ["1025", "2048"])
def test_gpu_worlds_meet_their_conditions(abi, name):
    """every world has inner nodes and no refused entry; under every move a quarter of the camera rays or more end on a flat primitive, and
    the set of first hits differs from the unmoved world's (so the frame does)"""
    from quad_rays import T_MAX
    from test_flat_bvh_gpu import _c_scene, _camera_rays
    sim = _sim(abi)
    sc, keep = _c_scene(abi, W, H)
    rays = _camera_rays(sc).reshape(-1, 6)
    base = U.world(name)
    nodes, order, n_always = sim.build(F.flats_array(abi, base, 1))
    assert nodes["count"][0] == 0 and n_always == 0
    b0, t0, _ = sim.hit(F.flats_array(abi, base, 1), rays, np.full(len(rays), T_MAX), True, 1)
    for mv in U.MOVES:
        for step in (1, 2, 3):
            quv = U.moved(base, mv, step)
            ok, _, _ = sim.entry_boxes(F.flats_array(abi, quv, 1))
            assert ok.all(), (mv, step)
            b, t, _ = sim.hit(F.flats_array(abi, quv, 1), rays, np.full(len(rays), T_MAX), True, 1)
            assert (b >= 1).mean() >= 0.25, (mv, step, (b >= 1).mean())
            assert (b != b0).mean() > 0.05 or (t != t0).mean() > 0.25, (mv, step)
    thin = U.needle(base, 100)
    ok, _, _ = sim.entry_boxes(F.flats_array(abi, thin, 1))
    assert (~ok).sum() == 1 and not ok[100]


# ------------------------------------------------------------------ the CLI, as far as it goes without a GPU
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")


def make_flat_anim():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_flat_anim", os.path.join(ROOT, "scenes", "make_flat_anim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("args, usage", [
    (["--flat-frames", "p_"], True),                                              # only with --frames
    (["--frames", "3", "--flat-frames"], True),                                   # a value is needed
    (["--frames", "3", "--flat-frames", ""], True),
    (["--frames", "3", "--flat-frames", "p_", "--flat-frames", "q_"], True),      # once
    (["--frames", "3", "--orbit", "0", "--flat-frames", "p_", "--denoise"], True),
    (["--flat-frames", "p_", "--passes", "2"], True),
    (["--frames", "3", "--flat-frames", "p_", "--passes", "2"], True),
    (["--flat-frames", "p_", "--adaptive", "0.1"], True),
    (["--frames", "3", "--flat-frames", "p_", "--adaptive", "0.1"], True),
    (["--frames", "3", "--flat-frames", "p_"], False),
    (["--frames", "3", "--flat-frames", "p_", "--orbit", "10"], False),
    (["--frames", "3", "--shutter", "0.5", "--flat-frames", "p_"], False),
    (["--flat-bvh", "--frames", "3", "--flat-frames", "p_", "--orbit", "0", "--shutter", "0"], False),
])
def test_flat_frames_flag_parsing(pkg, tmp_path, args, usage):
    """a refused command line prints the usage line and returns 0 before anything is read; an accepted one goes on to read the scene
    file — which does not exist here"""
    r = subprocess.run([EXE, str(tmp_path / "missing.json"), str(tmp_path / "out")] + args, capture_output=True, text=True, timeout=60)
    if usage:
        assert r.returncode == 0 and r.stdout.startswith("Usage:"), (args, r.returncode, r.stdout, r.stderr)
    else:
        assert r.returncode == 101 and "Unable to read config file" in r.stderr and "Usage" not in r.stdout, (args, r.returncode, r.stdout, r.stderr)


def test_flat_frame_files_are_checked_against_the_base_file(pkg, tmp_path):
    """frame 0's file is read and compared with the base file before a device is asked for: another count, shape or material, a file that
    is missing or not a scene — each ends the run with a message naming the frame.  A good file gets as far as the GPU."""
    gen = make_flat_anim()
    base, prefix = gen.write(str(tmp_path), n=4, frames=2, width=W, height=H, spp=2)
    good = json.load(open(prefix + "000.json"))
    assert [k for k, o in enumerate(good["objects"]) if "mesh" in o] == [3] and len(good["objects"][3]["mesh"]["faces"]) == 32

    def run(frame0):
        if frame0 is None:
            os.remove(prefix + "000.json") if os.path.exists(prefix + "000.json") else None
        else:
            open(prefix + "000.json", "w").write(frame0 if isinstance(frame0, str) else json.dumps(frame0))
        env = {k: v for k, v in os.environ.items() if k not in ("RT_GPUS", "RT_GPUS_EMULATE", "RT_ANIM")}
        return subprocess.run([EXE, base, str(tmp_path / "out"), "--frames", "2", "--orbit", "0", "--flat-frames", prefix], capture_output=True, text=True, timeout=60,
                              env=env)

    def variant(edit):
        cfg = json.loads(json.dumps(good))
        edit(cfg)
        return cfg

    five = json.loads(gen.make(5, 0.0, width=W, height=H, spp=2))
    quads = [{"q": {"x": k, "y": 1, "z": 0}, "u": {"x": 0.5, "y": 0, "z": 0}, "v": {"x": 0, "y": 0, "z": 0.5}, "material": good["objects"][3]["material"]} for k in range(32)]
    cases = {
        "count": (five, "50 flat primitives, the scene has 32"),
        "shape": (variant(lambda c: c["objects"].__setitem__(slice(3, 4), quads)), "flat primitive 0 has another shape"),
        "material": (variant(lambda c: c["objects"][3].__setitem__("material", {"Lambertian": {"albedo": [0.1, 0.2, 0.3]}})), "flat primitive 0 has another material"),
        "not json": ("{", ""),
        "missing": (None, ""),
    }
    for name, (frame0, needle) in cases.items():
        r = run(frame0)
        assert r.returncode == 101 and "frame 0 (" + prefix + "000.json)" in r.stderr and needle in r.stderr, (name, r.returncode, r.stdout, r.stderr)
        assert "Rendering" not in r.stdout, name
    r = run(good)                                    # the frame file is fine: the run gets to the device
    import torch
    if not torch.cuda.is_available():
        assert r.returncode == 101 and "frame 0" not in r.stderr and "render failed" in r.stderr, (r.stdout, r.stderr)
    else:
        assert r.returncode == 0 and r.stdout.count("Rendering") == 2, (r.stdout, r.stderr)
    # a base file without a flat primitive
    cfg = variant(lambda c: c["objects"].__delitem__(3))
    open(base, "w").write(json.dumps(cfg))
    r = run(good)
    assert r.returncode == 101 and "no flat primitive" in r.stderr
