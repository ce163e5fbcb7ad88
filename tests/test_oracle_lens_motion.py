"""The C oracle's lens and shutter (oracle/rt_oracle.h RtOracleExt) pinned on the CPU.

The extended oracle is the reference of tests/test_lens_motion_full_size.py, so it is itself checked here by what is independent
of it: the plain entry points (no extension: the same bits), the two Python restatements of the contract (LensMini of
tests/test_lens.py, MotionMini of tests/test_motion.py: bit for bit on every frame those tests use), known answers through the
camera hook, the accumulator's composition rule, and two committed fixtures."""
import ctypes as C
import os

import numpy as np
import pytest

import ext_scenes as X
import mini_oracle as M
from parity import assert_parity, pooled_atol
from test_lens import LENS_CASES, LensMini, _cfg
from test_motion import MOTION_CASES, NODE_TIME, TAU_LAST, MotionMini, _moving_cfg, tau_of
from test_progressive_reference import _resolve_ref

GOLDEN = os.path.join(X.ROOT, "tests", "golden")
COUNTERS = ("samples", "segments", "sphere_tests", "exact_tests", "tex_oob", "grid_steps", "segments_discarded", "n_gpus_used")
# (name, scene, w, h, spp, depth, seed) of the committed fixtures: tests/golden/make_golden.py's EXT_CASES
EXT_GOLDEN = {
    "cover_dof_96x64_spp4": (X.DOF, 96, 64, 4, 50, 0),
    "cover_motion_96x64_spp4": (X.MOTION_SCENE, 96, 64, 4, 50, 0),
}


def _ext_call(oracle, abi, sc, ext, x_range=None, tiles=None):
    """rt_oracle_render_window_ext itself (oracle.render goes to the plain entry point when it is given no extension)"""
    c = sc.c
    rows = abi.tiles_local_rows(c.height, tiles)
    rgb, lin, st = np.zeros((rows, c.width, 3), np.uint8), np.zeros((rows, c.width, 3), np.float32), abi.RtStats()
    x0, x1 = x_range or (0, c.width)
    rc = oracle.lib(abi).rt_oracle_render_window_ext(sc.ptr, C.byref(tiles) if tiles is not None else None, x0, x1,
                                                     C.byref(ext) if ext is not None else None, rgb.ctypes.data, lin.ctypes.data, C.byref(st), 0)
    assert rc == 0, rc
    return rgb, lin, st.as_dict()


def _accum_call(oracle, abi, sc, ext, begin, count):
    c = sc.c
    acc, st = np.zeros((c.height, c.width, 3), np.uint64), abi.RtStats()
    rc = oracle.lib(abi).rt_oracle_accumulate_ext(sc.ptr, None, 0, c.width, begin, count, C.byref(ext) if ext is not None else None,
                                                  acc.ctypes.data, C.byref(st), 0)
    assert rc == 0, rc
    return acc, st.as_dict()


def _same_frame(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: RGB8 differs at {int((got[0] != want[0]).sum())} values"
    a, b = got[1].view(np.uint32), want[1].view(np.uint32)
    assert np.array_equal(a, b), f"{what}: linear f32 bits differ at {int((a != b).sum())} values"


def _same_counters(got, want, what):
    for k in COUNTERS:
        assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.mark.parametrize("name,w,h,spp,depth", [("cover", 48, 32, 3, 50), ("test", 40, 30, 4, 8), ("cover4k_tex", 48, 27, 3, 50)])
def test_no_extension_is_the_plain_oracle_bit_for_bit(oracle, abi, load_scene, name, w, h, spp, depth):
    """ext NULL, an empty ext, center1 == every centre, lens_r == 0 (with and without the vectors), and all of them together:
    rt_oracle_render_window's RGB8, f32 bits and every counter; the same for rt_oracle_accumulate's words"""
    sc = load_scene(name, w, h, spp, depth=depth)
    want = oracle.render(abi, sc.ptr)
    want_acc = oracle.accumulate(abi, sc.ptr, 1, 2)
    still = X.centres(sc)
    u, v = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    exts = {"NULL": None, "empty": oracle.RtOracleExt()}
    keep = []
    for what, (c1, lens) in {"center1 == centres": (still, None), "lens_r == 0": (None, (u, v, 0.0)),
                             "both": (still, (u, v, 0.0)), "negative zero centres": (np.where(still == 0.0, -0.0, still), None)}.items():
        exts[what], k = oracle.make_ext(sc.ptr, c1, lens)
        keep.append(k)
    no_vectors = oracle.RtOracleExt()
    no_vectors.lens_r = 0.0
    exts["lens_r == 0 without vectors"] = no_vectors
    for what, ext in exts.items():
        got = _ext_call(oracle, abi, sc, ext)
        _same_frame(got, want, what)
        _same_counters(got[2], want[2], what)
        acc, st = _accum_call(oracle, abi, sc, ext, 1, 2)
        assert np.array_equal(acc, want_acc[0]), what
        _same_counters(st, want_acc[1], what)
    # a window of a row shard, through the binding's keyword arguments
    t = abi.RtRowTiles(2, 1, 3)
    a = oracle.render(abi, sc.ptr, tiles=t, x_range=(5, 29))
    b = oracle.render(abi, sc.ptr, tiles=t, x_range=(5, 29), center1=still, lens=(u, v, 0.0))
    _same_frame(b, a, "window of a shard")
    _same_counters(b[2], a[2], "window of a shard")


def _atan2(oracle, abi):
    L = oracle.lib(abi)
    return lambda y, x: L.rt_oracle_atan2(y, x)


@pytest.mark.parametrize("case", sorted(LENS_CASES))
def test_lens_frames_are_lensmini_bit_for_bit(oracle, abi, host, case):
    """every frame tests/test_lens.py compares the kernel with: the C oracle through a lens gives LensMini's bytes, f32 bits and
    segment count"""
    path, w, h, spp, depth, keys = LENS_CASES[case]
    sc, c1, lens = X.load(host, _cfg(path, **keys), w, h, spp, depth)
    assert c1 is None and lens[2] == keys["aperture"] / 2.0
    m_rgb, m_lin, m_segs = LensMini(sc.c, _atan2(oracle, abi), *lens).render()
    got = oracle.render(abi, sc.ptr, lens=lens)
    _same_frame(got, (m_rgb, m_lin), case)
    assert got[2]["segments"] == m_segs, (case, got[2]["segments"], m_segs)
    assert (got[2]["segments_discarded"] > 0) == (case == "lit")
    # (the lens does something: the pinhole frame of the same scene differs)
    assert not np.array_equal(oracle.render(abi, sc.ptr)[1], got[1])


@pytest.mark.parametrize("case", sorted(MOTION_CASES))
def test_motion_frames_are_motionmini_bit_for_bit(oracle, abi, host, case):
    """every frame tests/test_motion.py compares the kernel with (unlit, lit, textured, lens + motion): MotionMini's bytes, f32 bits
    and segment count"""
    path, w, h, spp, depth, moves, lens_keys = MOTION_CASES[case]
    rng = np.random.default_rng(500 + sorted(MOTION_CASES).index(case))   # (test_motion_frames_against_the_restatement's worlds)
    sc, c1, lens = X.load(host, _moving_cfg(path, rng, moves, lens_keys), w, h, spp, depth)
    assert c1 is not None and (lens is not None) == bool(lens_keys)
    m_rgb, m_lin, m_segs = MotionMini(sc.c, _atan2(oracle, abi), c1, lens).render()
    got = oracle.render(abi, sc.ptr, center1=c1, lens=lens)
    _same_frame(got, (m_rgb, m_lin), case)
    assert got[2]["segments"] == m_segs, (case, got[2]["segments"], m_segs)
    assert (got[2]["segments_discarded"] > 0) == case.startswith("lit")
    assert not np.array_equal(oracle.render(abi, sc.ptr, lens=lens)[1], got[1])   # motion does something


def _philox_x_v(c0, c1, c2, c3, seed):
    """word 0 of Philox4x32-10 over numpy arrays of counters (mini_oracle.philox4x32_10 vectorised; pinned against it below)"""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & np.uint64(M.M32) for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = seed & M.M32, (seed >> 32) & M.M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(M.M32),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(M.M32))
        k0, k1 = (k0 + 0x9E3779B9) & M.M32, (k1 + 0xBB67AE85) & M.M32
    return c0


def test_shutter_time_known_answers_and_both_ends_of_its_range(oracle, abi, load_scene):
    """tau through the hook against tau_of at a handful of (pixel, sample, seed), and at addresses that give tau = 0 and
    tau = 1 - 2^-24 EXACTLY: found by searching the 2048 x 2048 addresses (pixel, sample) of seed 0 (4.2 M addresses; the
    search finds one of each, so these are the true ends of the range, not the nearest the search came to)"""
    W = H = 2048
    sc = load_scene("cover", W, H, 1)
    for seed, pixel, s in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (7, 12345, 17), ((1 << 63) + 5, W * H - 1, 4095), (0xFFFFFFFF, 4099, 1 << 20)):
        sc.c.seed = seed
        o, d, tau = oracle.camera_ray(abi, sc.ptr, pixel % W, pixel // W, s)
        assert tau == tau_of(pixel, s, seed), (seed, pixel, s, tau)
        assert 0.0 <= tau < 1.0 and tau * 2.0 ** 24 == int(tau * 2.0 ** 24)
        # (no lens: the pinhole ray of the same jitter, and the ray does not depend on whether something moves)
        assert (o, d) == oracle.camera_ray(abi, sc.ptr, pixel % W, pixel // W, s, center1=X.centres(sc) + 1.0)[:2]
    sc.c.seed = 0
    pix, smp = np.arange(2048, dtype=np.uint64)[:, None], np.arange(2048, dtype=np.uint64)[None, :]
    x = _philox_x_v(pix, smp, NODE_TIME, 0, 0)
    assert int(x[5, 9]) == M.philox4x32_10(5, 9, NODE_TIME, 0, 0, 0)[0] and int(x[2047, 3]) == M.philox4x32_10(2047, 3, NODE_TIME, 0, 0, 0)[0]
    q = x >> np.uint64(8)
    first, last = np.argwhere(q == 0), np.argwhere(q == (1 << 24) - 1)
    assert len(first) and len(last), (int(q.min()), int(q.max()))
    for (pixel, s), want in ((first[0], 0.0), (last[0], TAU_LAST)):
        pixel, s = int(pixel), int(s)
        assert tau_of(pixel, s, 0) == want
        assert oracle.camera_ray(abi, sc.ptr, pixel % W, pixel // W, s)[2] == want, (pixel, s)
    print(f"tau = 0 at (pixel, sample) {first[0].tolist()}, tau = 1 - 2^-24 at {last[0].tolist()} (seed 0)")


def _lens_attempts(pixel, s, seed):
    """Philox calls the lens draw of (pixel, s) needs, by the contract (candidates (x, y) then (z, w) of attempts 0, 1, ...)"""
    a = 0
    while True:
        w = M.philox4x32_10(pixel, s, M.NODE_CAMERA, 1 + a, seed & M.M32, (seed >> 32) & M.M32)
        if any(M.range_m1_1(p) ** 2 + M.range_m1_1(q) ** 2 < 1.0 for p, q in ((w[0], w[1]), (w[2], w[3]))):
            return a + 1
        a += 1


def test_lens_rays_needing_a_second_and_a_third_philox_call(oracle, abi, host):
    """the camera ray through the hook against LensMini.camera_ray, origin and direction bit for bit: at ordinary addresses, at
    addresses whose first candidate misses the disc, and at ones that need a second (4.6 %) and a third (0.2 %) Philox call"""
    sc, _, lens = X.load(host, _cfg(X.COVER, aperture=0.6, focus_dist=4.5), 64, 40, 8, 8)
    W = sc.c.width
    mini = LensMini(sc.c, _atan2(oracle, abi), *lens)
    moving = MotionMini(sc.c, _atan2(oracle, abi), X.centres(sc) + 0.5, lens)
    by_calls = {1: [], 2: [], 3: []}
    for pixel in range(W * sc.c.height):
        for s in range(sc.c.samples_per_pixel):
            n = _lens_attempts(pixel, s, sc.c.seed)
            if n in by_calls and len(by_calls[n]) < 6:
                by_calls[n].append((pixel, s))
        if len(by_calls[3]) >= 2 and len(by_calls[2]) >= 6:
            break
    assert len(by_calls[2]) >= 6 and len(by_calls[3]) >= 2, {k: len(v) for k, v in by_calls.items()}
    bits = lambda v: np.array(v, np.float64).view(np.uint64).tolist()
    for n, addrs in by_calls.items():
        for pixel, s in addrs:
            x, y = pixel % W, pixel // W
            o, d, tau = oracle.camera_ray(abi, sc.ptr, x, y, s, lens=lens)
            for m in (mini, moving):
                m.pixel, m.sample = pixel, s
                mo, md = m.camera_ray(x, y)
                assert bits(o) == bits(mo) and bits(d) == bits(md), (n, pixel, s)
            assert tau == tau_of(pixel, s, sc.c.seed)
            assert o != tuple(sc.c.cam_origin)   # (the ray does leave the lens, not its centre)


def test_refusals(oracle, abi, host, load_scene):
    """a moving Light, a center1 - center that is not finite, a bad lens radius, a lens without its vectors: RT_ERR_INVALID from
    every entry point, and the buffers untouched"""
    sc = load_scene("test", 12, 9, 2, depth=6)
    still = X.centres(sc)
    light = sc.lights()[0]
    other = next(i for i in range(sc.c.n_spheres) if i != light)
    moved_light, inf, nan, overflow = still.copy(), still.copy(), still.copy(), still.copy()
    moved_light[light, 1] += 0.25
    inf[other, 0] = np.inf
    nan[other, 2] = np.nan
    overflow[other, 0], big = 1.7e308, host.Scene.load(X.TEST)
    u, v = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    bad = [dict(center1=moved_light), dict(center1=inf), dict(center1=nan), dict(lens=(u, v, -0.1)), dict(lens=(u, v, float("nan"))),
           dict(lens=(u, v, float("inf")))]
    for kw in bad:
        for call in (lambda: oracle.render(abi, sc.ptr, **kw), lambda: oracle.accumulate(abi, sc.ptr, 0, 1, **kw),
                     lambda: oracle.camera_ray(abi, sc.ptr, 1, 1, 0, **kw)):
            with pytest.raises(RuntimeError, match="failed: %d" % abi.RT_ERR_INVALID):
                call()
    # c1 - c0 that overflows although both are finite
    big.c.spheres[other].center[0] = -1.7e308
    big.c.width, big.c.height, big.c.samples_per_pixel = 4, 3, 1
    with pytest.raises(RuntimeError):
        oracle.render(abi, big.ptr, center1=overflow)
    no_vectors = oracle.RtOracleExt()
    no_vectors.lens_r = 0.1
    rgb = np.full((9, 12, 3), 7, np.uint8)
    rc = oracle.lib(abi).rt_oracle_render_window_ext(sc.ptr, None, 0, 12, C.byref(no_vectors), rgb.ctypes.data, None, None, 0)
    assert rc == abi.RT_ERR_INVALID and (rgb == 7).all()
    # what is allowed: the light named in center1 at its own place, a static sphere beside movers
    ok = still.copy()
    ok[other, 0] += 0.5
    assert oracle.render(abi, sc.ptr, center1=ok)[2]["segments"] > 0


@pytest.mark.parametrize("case", ["lit_lens", "textured", "bouncing_lens"])
def test_accumulate_ext_composes_and_resolves_to_the_frame(oracle, abi, host, case):
    """sample ranges of rt_oracle_accumulate_ext, in any split and order, add up to the words of one call (paths and counters
    too), and those words resolve to rt_oracle_render_window_ext's frame within the pooled bar, as
    tests/test_progressive_reference.py holds the plain pair to"""
    path, w, h, _, depth, moves, lens_keys = MOTION_CASES[case]
    n = 7
    rng = np.random.default_rng(500 + sorted(MOTION_CASES).index(case))
    sc, c1, lens = X.load(host, _moving_cfg(path, rng, moves, lens_keys), w, h, n, depth)
    kw = dict(center1=c1, lens=lens)
    whole, st = oracle.accumulate(abi, sc.ptr, 0, n, **kw)
    for split in ([(0, 1), (1, n)], [(4, n), (0, 2), (2, 4)], [(s, s + 1) for s in range(n - 1, -1, -1)]):
        acc, tot = None, dict.fromkeys(("segments", "segments_discarded", "tex_oob", "samples"), 0)
        for b, e in split:
            acc, s = oracle.accumulate(abi, sc.ptr, b, e - b, accum=acc, **kw)
            for k in tot:
                tot[k] += s[k]
        assert np.array_equal(acc, whole), (case, split)
        assert all(tot[k] == st[k] for k in tot), (case, split, tot, st)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr, **kw)
    rgb, lin = _resolve_ref(whole.ravel(), n)
    assert_parity(rgb.reshape(o_rgb.shape), lin.reshape(o_lin.shape), o_rgb, o_lin, f"{case}: accumulate_ext [0, {n}) resolved", atol=pooled_atol(n))
    for k in ("segments", "segments_discarded", "tex_oob", "samples"):
        assert st[k] == o_st[k], (case, k, st[k], o_st[k])
    # a range that does not start at 0 is not the range that does (the sample index reaches tau and the lens point)
    assert not np.array_equal(oracle.accumulate(abi, sc.ptr, 3, 2, **kw)[0], oracle.accumulate(abi, sc.ptr, 0, 2, **kw)[0])
    # a window of a row shard addresses the same words
    t = abi.RtRowTiles(2, 1, 3)
    rows = abi.tiles_global_rows(h, t)
    part, _ = oracle.accumulate(abi, sc.ptr, 0, n, tiles=t, x_range=(3, 11), **kw)
    assert np.array_equal(part[:, 3:11], whole[rows, 3:11]) and not part[:, :3].any() and not part[:, 11:].any()


@pytest.mark.parametrize("name", sorted(EXT_GOLDEN))
def test_extended_oracle_matches_its_golden_frames(oracle, abi, host, name):
    """the shipped depth-of-field and motion-blur scenes at 96 x 64, spp 4, as tests/golden/make_golden.py froze them: every
    operation is IEEE, so bytes, f32 bits and counters are the same on any machine"""
    path, w, h, spp, depth, seed = EXT_GOLDEN[name]
    sc, c1, lens = X.load(host, path, w, h, spp, depth, seed)
    assert (c1 is not None) == ("motion" in name) and (lens is not None) == ("dof" in name)
    rgb, lin, st = oracle.render(abi, sc.ptr, center1=c1, lens=lens)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert st["samples"] == int(g["samples"]) == w * h * spp
    assert st["segments"] == int(g["segments"]) and st["segments_discarded"] == int(g["segments_discarded"]) == 0
    assert np.array_equal(rgb, g["rgb8"]) and np.array_equal(lin.view(np.uint32), g["linear"].view(np.uint32))
    # and the fixture is not the plain scene's frame
    assert not np.array_equal(oracle.render(abi, sc.ptr)[1], lin)
