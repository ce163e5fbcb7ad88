"""Flat primitives that emit and are sampled without a GPU: the schema of "emit"; the host build of csrc/common/rt_flat_light.h
against the restatement (tests/flat_light_mini.py) bit for bit on 10^5 activations per class; the uniformity of the aim points; the CPU build
of the lit QUADS lane code (tests/flatlight/flat_light_sim.cpp) against FlatLightMini on the parity frames; the umbra / penumbra check of the
GPU test on that build; and the host code under ASan and UBSan as a stand-alone program."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import flat_light_frames as LF
import flat_light_mini as LM
import flat_light_sim
import mini_oracle as M
from parity import assert_parity, pooled_atol
from test_medium_gpu import _cfg, _lam, _load, _obj
from test_quad_gpu import _box, _quad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = _lam(0.5, 0.5, 0.5)
TRI = {"triangle": [[0, 0, 1], [1, 0, 1], [0, 1, 1]], "material": LAM}
MESH = {"mesh": {"vertices": [[0, 0, 2], [1, 0, 2], [0, 1, 2], [1, 1, 2]], "faces": [[0, 1, 2], [1, 3, 2]]}, "material": LAM}
QUAD = _quad((0, 0, 0), (1, 0, 0), (0, 1, 0), LAM)
BOX = _box((1, 1, 1), (2, 2, 2), LAM)


def _with(o, **kw):
    o = json.loads(json.dumps(o))
    o.update(kw)
    return o


def _loads(host, objs):
    return host.Scene.loads(json.dumps(_cfg(objs, sky=False)))


# ------------------------------------------------------------------ schema
def test_the_key_on_each_of_the_four_forms(host, abi):
    """a quad, a "triangle", a "box" (its six quads, each with the key) and a "mesh" (every face); both point forms; an entry without the key
    is three zeros; a file without the key has no table"""
    sc = _loads(host, [_with(QUAD, emit=[1.0, 0.9, 0.75]), _obj((0, 0, -3), 1.0, LAM), _with(TRI, emit={"x": 0.1, "y": 0.2, "z": 0.3}), QUAD,
                       _with(BOX, emit=[0, 0.5, 0]), _with(MESH, emit=[0.25, 0, 1])])
    e = sc.flat_emit()
    assert e.dtype == np.float32 and e.shape == (11, 3) and len(sc.quads()) == 11
    want = np.array([[1.0, 0.9, 0.75], [0.1, 0.2, 0.3], [0, 0, 0]] + [[0, 0.5, 0]] * 6 + [[0.25, 0, 1]] * 2, np.float32)
    assert e.tobytes() == want.tobytes()
    assert _loads(host, [QUAD, TRI, BOX, MESH]).flat_emit() is None
    assert abi.RT_MAX_FLAT_LIGHTS == 32


@pytest.mark.parametrize("objs,needle", [
    ([QUAD, _with(QUAD, emit=[1.5, 0, 0])], "objects[1]"),
    ([_with(TRI, emit=[0, -0.1, 0])], "objects[0]"),
    ([QUAD, QUAD, _with(BOX, emit=[0, 0, 1.0000000000000002])], "objects[2]"),
    ([_with(MESH, emit=[0, 0])], "objects[0]"),
    ([_with(MESH, emit="red")], "objects[0]"),
    ([QUAD, _obj((0, 0, 0), 1.0, LAM) | {"emit": [1, 1, 1]}], "objects[1]"),
    ([_with(QUAD, emit=[1, 1, 1], move=[0, 0.5, 0])], "objects[0]"),
    ([TRI, _with(BOX, emit=[0.5, 0.5, 0.5], move={"x": 0, "y": 0, "z": 1e-300})], "objects[1]"),
])
def test_load_errors_name_their_object(host, objs, needle):
    with pytest.raises(host.RtError) as e:
        _loads(host, objs)
    assert needle in str(e.value) and ("emit" in str(e.value)), str(e.value)


def test_a_duplicate_key_is_a_load_error(host):
    text = json.dumps(_cfg([QUAD, _with(QUAD, emit=[1, 1, 1])], sky=False)).replace('"emit": [1, 1, 1]', '"emit": [1, 1, 1], "emit": [0, 0, 0]')
    assert text.count('"emit"') == 2
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(text)
    assert "objects[1]" in str(e.value) and "duplicate field `emit`" in str(e.value)


def test_emit_with_a_zero_move_or_zero_emit_with_a_move_loads(host):
    sc = _loads(host, [_with(QUAD, emit=[1, 1, 1], move=[0, 0, 0]), _with(TRI, emit=[0, 0, 0], move=[0, 1, 0])])
    assert sc.flat_emit().tolist() == [[1, 1, 1], [0, 0, 0]] and sc.flat_motion().tolist() == [[0, 0, 0], [0, 1, 0]]


def test_round_trip_is_bit_for_bit_and_a_file_without_the_key_keeps_its_bytes(host):
    rng = np.random.default_rng(3)
    vals = rng.random((4, 3)).astype(np.float32)
    vals[1] = (np.float32(1.0), np.float32(np.nextafter(np.float32(1.0), np.float32(0.0))), np.float32(1e-45))
    objs = [_with(QUAD, emit=[float(x) for x in vals[0]]), _with(TRI, emit=[float(x) for x in vals[1]]), QUAD, _with(BOX, emit=[float(x) for x in vals[2]]),
            _with(MESH, emit=[0, 0, 0])]
    a = _loads(host, objs)
    text = a.to_json()
    b = host.Scene.loads(text)
    assert a.flat_emit().tobytes() == b.flat_emit().tobytes() and b.to_json() == text
    assert text.count('"emit"') == 1 + 1 + 6 + 2                  # only where the file had it: the plain quad has none, the mesh's zeros are written
    plain = _loads(host, [QUAD, TRI, BOX, MESH]).to_json()
    assert "emit" not in plain
    assert _loads(host, [_with(QUAD, emit=[0, 0, 0]), TRI, BOX, MESH]).to_json().replace(',"emit":[0.0,0.0,0.0]', "") == plain


def test_the_example_file_is_what_its_script_writes(host):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cornell_panel_scene", os.path.join(ROOT, "scenes", "make_cornell_panel_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make() == open(os.path.join(ROOT, "scenes", "cornell_panel_600x600_spp128.json")).read()
    sc = host.Scene.load(os.path.join(ROOT, "scenes", "cornell_panel_600x600_spp128.json"))
    e = sc.flat_emit()
    assert len(sc.lights()) == 0 and (e != 0).any(axis=1).sum() == 1 and e[(e != 0).any(axis=1)][0].tolist() == [1.0, np.float32(0.9), 0.75]


# ------------------------------------------------------------------ the aim, bit for bit
N = 100_000


def _words_of(a53, b53):
    """the four words that give a = a53 2^-53 and b = b53 2^-53 (the low 11 bits of each 64-bit word are free: zero here)"""
    a, b = a53.astype(np.uint64) << np.uint64(11), b53.astype(np.uint64) << np.uint64(11)
    m = np.uint64(0xFFFFFFFF)
    return np.stack([a & m, a >> np.uint64(32), b & m, b >> np.uint64(32)], axis=1).astype(np.uint32)


def aim_classes(seed=11):
    """{class: (quv [N, 9], triangle [N], words [N, 4])}: what the host build and the restatement are compared on"""
    rng = np.random.default_rng(seed)
    words = lambda: rng.integers(0, 2 ** 32, (N, 4), dtype=np.uint64).astype(np.uint32)
    quv = lambda s=4.0: rng.uniform(-s, s, (N, 9))
    tri = (np.arange(N) & 1).astype(np.int32)
    out = {"parallelogram": (quv(), np.zeros(N, np.int32), words()), "triangle": (quv(), np.ones(N, np.int32), words())}
    a53 = rng.integers(0, 2 ** 53, N, dtype=np.uint64)
    b53 = (np.uint64(2 ** 53) - a53 + (np.arange(N, dtype=np.uint64) % np.uint64(9)) - np.uint64(4)) & np.uint64(2 ** 53 - 1)
    out["a + b at 1"] = (quv(), np.ones(N, np.int32), _words_of(a53, b53))
    ext = np.array([0, 2 ** 53 - 1, 1, 2 ** 52], np.uint64)
    w = words()
    wa, wb = _words_of(ext[rng.integers(0, 4, N)], ext[rng.integers(0, 4, N)]), w.copy()
    w[::2, :2] = wa[::2, :2]                                   # a at an extreme, b free
    w[1::2, 2:] = wa[1::2, 2:]                                 # b at an extreme, a free
    w[::5] = wa[::5]                                           # both
    w[:, 0] |= wb[:, 0] & np.uint32(0x7FF); w[:, 2] |= wb[:, 2] & np.uint32(0x7FF)      # (the free low bits: any value)
    out["0 and the largest value below 1"] = (quv(), tri, w)
    g = quv()
    g[::2, 6:9] = g[::2, 3:6] * (1.0 + 1e-12 * rng.uniform(-1, 1, (N // 2, 1)))         # needles: v nearly u
    g[1::2, 6:9] = g[1::2, 3:6] * 1e-9 + rng.uniform(-1e-3, 1e-3, (N // 2, 3))          # skewed: one short edge
    out["needle and skewed"] = (g, tri, words())
    big = quv()
    big[::2] *= 10.0 ** rng.uniform(150, 152, (N // 2, 1))
    big[1::2] *= 10.0 ** rng.uniform(-152, -150, (N // 2, 1))
    out["|Q|, |u| over 1e+-150"] = (big, tri, words())
    return out


@pytest.mark.parametrize("name", ["parallelogram", "triangle", "a + b at 1", "0 and the largest value below 1", "needle and skewed", "|Q|, |u| over 1e+-150"])
def test_host_aim_against_the_restatement_bit_for_bit(abi, name):
    quv, tri, words = aim_classes()[name]
    got = flat_light_sim.load(abi).aim(quv, tri, words)
    rows, wl = quv.tolist(), words.tolist()
    want = np.array([LM.aim(r[0:3], r[3:6], r[6:9], bool(t), w) for r, t, w in zip(rows, tri.tolist(), wl)])
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got.view(np.uint64) != want.view(np.uint64)).any(axis=1).sum())
    ab = flat_light_sim.load(abi).ab(words)
    assert (ab >= 0.0).all() and (ab < 1.0).all()
    if name == "a + b at 1":
        s = ab[:, 0] + ab[:, 1]
        assert (s > 1.0).sum() > N // 4 and (s <= 1.0).sum() > N // 4 and (s == 1.0).sum() > N // 20      # both sides and the tie
    if name == "0 and the largest value below 1":
        assert (ab == 0.0).any() and (ab == 1.0 - 2.0 ** -53).any()


def test_the_draw_is_the_childs_slot_all_ones(abi):
    """rng(pixel, sample, child_node(node, j), 0xFFFFFFFF): the C build's words against the Python Philox"""
    rng = np.random.default_rng(5)
    act = rng.integers(0, 2 ** 32, (2000, 4), dtype=np.uint64).astype(np.uint32)
    act[:, 3] %= 40
    seed = 0x1234_5678_9ABC_DEF0
    got = flat_light_sim.load(abi).words(act, seed)
    for (px, s, node, j), w in zip(act.tolist(), got.tolist()):
        assert tuple(w) == M.philox4x32_10(px, s, M.child_node(node, j), LM.AIM_SLOT, seed & M.M32, seed >> 32)


def _chi2_quantile(dof):
    """the 1 - 1e-6 quantile of chi-square with `dof` degrees of freedom"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, dof))
    except ImportError:
        # scipy.stats.chi2.ppf(1 - 1e-6, 15) = 56.4934...: the root of the regularised upper incomplete gamma Q(7.5, x / 2) = 1e-6
        assert dof == 15
        return 56.49344249969959


@pytest.mark.parametrize("triangle", [False, True])
def test_aim_points_are_uniform(abi, triangle):
    """65 536 consecutive (pixel, sample) addresses on one entry, binned into 16 equal-area cells of (a, b): the unit square 4 x 4; the
    triangle a + b <= 1 by the map (a, b) -> (s, t) = ((a + b)^2, a / (a + b)), which is uniform on the unit square for a uniform point of
    the triangle, 4 x 4.  The chi-square statistic (15 degrees of freedom) is below the 1 - 1e-6 quantile.  Without the fold the points of
    a "triangle" fill the whole square and half of them fall outside it: the statistic explodes (asserted)."""
    sim = flat_light_sim.load(abi)
    act = np.zeros((65536, 4), np.uint32)
    act[:, 0] = np.arange(65536) // 64 + 1000
    act[:, 1] = np.arange(65536) % 64
    act[:, 2], act[:, 3] = 2, 1
    words = sim.words(act, 77)
    quv = np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (len(act), 1))     # T = (a, b, 0) exactly
    T = sim.aim(quv, np.full(len(act), int(triangle), np.int32), words)
    a, b = T[:, 0], T[:, 1]

    def statistic(a, b):
        if triangle:
            s = a + b
            inside = s <= 1.0
            u, v = s * s, np.divide(a, s, out=np.zeros_like(a), where=s > 0)
            cell = np.where(inside, np.minimum((u * 4).astype(int), 3) * 4 + np.minimum((v * 4).astype(int), 3), 16)
        else:
            cell = np.minimum((a * 4).astype(int), 3) * 4 + np.minimum((b * 4).astype(int), 3)
        counts = np.bincount(cell, minlength=17)
        expect = len(a) / 16.0
        return float(((counts[:16] - expect) ** 2 / expect).sum() + counts[16] ** 2 / expect)       # (a point outside the triangle: its own penalty)
    x2, bound = statistic(a, b), _chi2_quantile(15)
    print(f"triangle={triangle}: chi-square {x2:.2f}, bound {bound:.2f}")
    assert x2 < bound
    if triangle:
        raw = sim.ab(words)
        assert statistic(raw[:, 0], raw[:, 1]) > 100 * bound, "the fold dropped must fail"


# ------------------------------------------------------------------ the lane code
@pytest.mark.parametrize("case", LF.CPU_CASES)
def test_lane_code_against_the_restatement(pkg, abi, oracle, host, case):
    """the CPU build of the lit QUADS lane code on the parity frames: tests/parity.py's bar and the exact segment count, through the scan
    and through the structure (bit for bit the scan)"""
    sim = flat_light_sim.load(abi)
    sc, c1, lens, quads, normals, emit = LF.world(host, case)
    m = LF.mini_frame(oracle, abi, host, case)
    rc, rgb, lin, segs, info = sim.render(sc.c, quads, emit, normals, c1, lens=lens)
    assert (lens is not None) == (case == "lens")
    assert rc == 0 and info[0] & flat_light_sim.FLAT_LIGHTS_BIT and info[1] == int((emit != 0).any(axis=1).sum()) and info[2] == m["n_lights"]
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(LF.SPP))
    assert segs == m["segments"] - m["discarded"]
    rc, rgb2, lin2, segs2, info2 = sim.render(sc.c, quads, emit, normals, c1, flat_bvh=True, lens=lens)
    assert rc == 0 and info2[0] & flat_light_sim.FLAT_BVH_BIT and segs2 == segs
    assert np.array_equal(lin.view(np.uint32), lin2.view(np.uint32)) and np.array_equal(rgb, rgb2)
    # no emitter: the world is the one that never had any (no bit, the sphere lights alone) and renders another frame
    rc, _, lin0, _, info0 = sim.render(sc.c, quads, np.zeros_like(emit), normals, c1, lens=lens)
    rc1, _, lin1, _, info1 = sim.render(sc.c, quads, None, normals, c1, lens=lens)
    assert rc == 0 and rc1 == 0 and info0 == info1 and not info0[0] & flat_light_sim.FLAT_LIGHTS_BIT and info0[1] == 0
    assert np.array_equal(lin0.view(np.uint32), lin1.view(np.uint32)) and not np.array_equal(lin0.view(np.uint32), lin.view(np.uint32))


@pytest.mark.parametrize("case", ["room_panel", "tri_lamp"])
def test_first_hit_records_of_an_emitter(pkg, abi, oracle, host, case):
    """AOV and surface records bitwise: a first hit on an emitter is albedo `emit`, kind RT_MAT_LIGHT"""
    sim = flat_light_sim.load(abi)
    sc, c1, lens, quads, normals, emit = LF.world(host, case)
    mini = LF.mini(oracle, abi, sc, c1, lens, quads, normals, emit)
    rc, aov, surf = sim.aovs(sc.c, quads, LF.SPP, emit, normals, c1)
    assert rc == 0
    want = mini.aovs(LF.SPP)
    assert np.array_equal(aov.view(np.uint32), want.view(np.uint32))
    ids, kinds, ts = mini.surface()
    assert np.array_equal(surf["id"], ids) and np.array_equal(surf["kind"], kinds) and np.array_equal(surf["t"].view(np.uint64), ts.view(np.uint64))
    k = int(np.nonzero((emit != 0).any(axis=1))[0][0])
    on_lamp = surf["id"] == sc.c.n_spheres + k
    assert on_lamp.sum() >= 4 and (surf["kind"][on_lamp] == abi.RT_MAT_LIGHT).all()
    assert (np.abs(aov[..., :3] - emit[k]).max(axis=2) == 0).any()


@pytest.mark.parametrize("case", ["room_panel", "panel_sphere", "box_lamp"])
def test_tables_through_the_c_structs(abi, host, case):
    """rt_tables.h build_flat_lights — the code rt_hip_scene_set_flat_lights uploads from — on the host: no emitter gives the tables of a world
    that never had the call, byte for byte; with emitters only their own records of `mat` and `matc` (kind Light, colour emit, every other
    byte zero) and the light list (the Light spheres, then object ids n_spheres + k in entry order) change; all zeros restores every table"""
    sim = flat_light_sim.load(abi)
    sc, c1, lens, quads, normals, emit = LF.world(host, case)
    n_sph, n = sc.c.n_spheres, len(quads)
    rc0, never, info0 = sim.tables(sc.c, quads, None)
    rc1, zeros, info1 = sim.tables(sc.c, quads, np.zeros_like(emit))
    rc2, lit, info2 = sim.tables(sc.c, quads, emit)
    assert rc0 == rc1 == rc2 == 0 and never == zeros and info0 == info1 and not info0[0] & flat_light_sim.FLAT_LIGHTS_BIT
    emitters = np.nonzero((emit != 0).any(axis=1))[0].tolist()
    sphere_lights = np.frombuffer(never["lights"], np.uint32).tolist()
    assert sphere_lights == host.Scene.lights(sc) and info2 == [info0[0] | flat_light_sim.FLAT_LIGHTS_BIT, len(emitters), len(sphere_lights) + len(emitters)]
    assert np.frombuffer(lit["lights"], np.uint32).tolist() == sphere_lights + [n_sph + k for k in emitters]
    for name in ("mat", "matc"):
        size = len(lit[name]) // (n_sph + n)
        assert size in (80, 48) and size * (n_sph + n) == len(lit[name]) == len(never[name])
        a, b = np.frombuffer(lit[name], np.uint8).reshape(n_sph + n, size), np.frombuffer(never[name], np.uint8).reshape(n_sph + n, size)
        assert np.nonzero((a != b).any(axis=1))[0].tolist() == [n_sph + k for k in emitters], name
        for k in emitters:
            rec = a[n_sph + k].tobytes()
            assert rec[:12] == emit[k].tobytes() and np.frombuffer(rec[12:16], np.uint32)[0] == abi.RT_MAT_LIGHT and not any(rec[16:]), (name, k)


def test_refused_tables_name_their_entry(abi, host):
    sim = flat_light_sim.load(abi)
    sc, c1, lens, quads, normals, emit = LF.world(host, "room_panel")
    for k, v in ((7, np.nan), (2, 1.5), (4, -1e-9), (0, np.inf)):
        bad = emit.copy(); bad[9, 0] = 7.0; bad[k, 1] = v
        rc, _, _, _, info = sim.render(sc.c, quads, bad, normals, c1)
        assert rc == 2 and info[1] == k
        assert LM.emit_check(bad)[0] == k == sim.emit_check(bad)[0]
    assert sim.emit_check(emit) == (len(emit), 1) and LM.emit_check(emit) == (len(emit), [int(np.nonzero((emit != 0).any(axis=1))[0][0])])


def test_umbra_and_penumbra_on_the_lane_build(abi, host):
    """tests/test_flat_light_gpu.py::test_umbra_and_penumbra on the CPU build (the break — rt_flat_light_aim returning the panel's centre —
    was made once on this build, and this test failed)"""
    sc, c1, lens = _load(host, LF.shadow_cfg(), LF.SHADOW_W, LF.SHADOW_H, LF.SHADOW_SPP, 8, seed=29)
    rc, rgb, lin, segs, info = flat_light_sim.load(abi).render(sc.c, sc.quads(), sc.flat_emit())
    assert rc == 0 and info[1] == 1
    print(LF.check_shadow(sc.c, rgb, lin))


# ------------------------------------------------------------------ sanitizers
def test_flat_light_host_code_under_asan_and_ubsan(tmp_path):
    """tests/flatlight/flat_light_main.cpp, built with ASan + UBSan as a stand-alone program (its own main, no Python in the process)"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    exe = tmp_path / "flat_light_main"
    hostdir = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "flatlight", "flat_light_main.cpp"), os.path.join(hostdir, "scene.cpp"),
                    os.path.join(hostdir, "jpeg.cpp"), "-I", os.path.join(ROOT, "include"), "-lz", "-lpthread", "-o", str(exe)], check=True)
    for seed in (1, 2):
        r = subprocess.run([str(exe), str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-2000:])
        assert "none outside" in r.stdout and "round trip of 11 entries" in r.stdout and "structure == scan" in r.stdout, r.stdout
        print(r.stdout.strip())
