"""Progressive rendering against references that share no code with it.

tests/test_progressive.py pins the accumulating kernels and rt_resolve against the one-shot frame, which comes from the same
kernel and the same rt_core.h fixed-point functions.  This module compares them with independent restatements instead:

  - oracle.accumulate (oracle/rt_oracle.c rt_oracle_accumulate): the CPU oracle's sample loop at ANY sample index, added into
    u64 words by the rule include/rt_abi.h states — written from that text, not from rt_core.h;
  - exact rational arithmetic (fractions.Fraction) for what a resolve of a word must give;
  - hostsim_resolve (tests/hostsim): rt_core.h's resolve arithmetic compiled for the CPU, the bit-exact target of rt_resolve
    once it has itself been checked against the exact arithmetic.

Sample indices up to 2^23 - 2, accumulators at their 2^23 - 1 sample limit, a caller's non-zero words (carries between the
dwords, NaN flags already set), odd pixel counts and unaligned RGB8 buffers (rt_resolve's byte stores) and option changes
between passes are covered here; none of them is reached by the one-shot comparisons."""
import bisect
import ctypes as C
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from parity import LINEAR_ATOL, assert_parity, pooled_atol
from test_progressive import _accumulate, _assert_identical, _cli, _new_accum, _one_shot, _resolve, _split_equals_one_shot, _stream

F = 1 << 63               # sticky NaN flag of an accumulator word
ONE = 1 << 40             # a sample of value 1.0 in 2^-40 fixed point
MAX_SAMPLES = (1 << 23) - 1
NS = (1, 2, 3, 7, 255, 8191, 8192, (1 << 20) + 1, MAX_SAMPLES)
# sample ranges of the high-index tests: low, around 2^16 (a kernel that kept 16 bits of the base), 2^20 + 5, the very top
RANGES = ((0, 24), ((1 << 16) - 12, (1 << 16) + 12), ((1 << 20) + 5, (1 << 20) + 29), (MAX_SAMPLES - 24, MAX_SAMPLES))


# ---------------------------------------------------------------------------------------------------- references

def _f32_to_u8(x):
    """raytracer.rs:213's palette conversion over an array, restated like rt_oracle_f32_to_u8: round-half-even of
    min(x * 255, 255) in f32, non-positive -> 0, NaN -> 255 (checked against rt_oracle_f32_to_u8 below)"""
    s = np.asarray(x, np.float32) * np.float32(255.0)
    out = np.rint(np.clip(np.nan_to_num(s, nan=255.0), 0.0, 255.0))
    return out.astype(np.uint8)


def _resolve_ref(words, n):
    """an accumulator holding n samples per pixel -> (RGB8, linear): the mean of the sum in f64, rounded to f32"""
    w = np.asarray(words, np.uint64)
    lin = (((w & np.uint64(F - 1)).astype(np.float64) / float(ONE)) / n).astype(np.float32)
    lin[(w & np.uint64(F)) != 0] = np.nan
    return _f32_to_u8(np.sqrt(lin)), lin


def _f32_rn(q):
    """q (a non-negative Fraction) rounded to the nearest f32, ties to even"""
    f = np.float32(float(q))   # float(Fraction) is correctly rounded; one more rounding leaves it within 1 ulp of the answer
    cands = [c for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))) if c >= 0]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(np.array(c).view(np.uint32)) & 1))


# boundaries of the exact byte: round(255 sqrt(q)) goes from k - 1 to k at sqrt(q) = (k - 0.5) / 255
BOUNDS = [Fraction(2 * k - 1, 510) ** 2 for k in range(1, 256)]


def _exact_byte(q):
    """round-half-even of min(255 sqrt(q), 255), exactly"""
    below = bisect.bisect_left(BOUNDS, q)     # boundaries strictly below q
    if below < 255 and BOUNDS[below] == q:    # on a boundary: 255 sqrt(q) = k - 0.5 exactly, k = below + 1
        return below + 1 if (below + 1) % 2 == 0 else below
    return below


@pytest.fixture(scope="module")
def resolve_lib(hostsim):
    hostsim.hostsim_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    hostsim.hostsim_resolve.restype = None

    def run(words, n, want_rgb=True, want_lin=True):
        w = np.ascontiguousarray(words, np.uint64)
        assert w.size % 3 == 0
        rgb = np.zeros(w.size, np.uint8) if want_rgb else None
        lin = np.zeros(w.size, np.float32) if want_lin else None
        hostsim.hostsim_resolve(w.ctypes.data, n, w.size // 3, rgb.ctypes.data if want_rgb else None, lin.ctypes.data if want_lin else None)
        return rgb, lin
    return run


def _crafted_words(n, resolve_lib):
    """the word set of the resolve tests for n samples per pixel (a multiple of 3 words: whole pixels)"""
    rng = np.random.default_rng(1000 + n)
    ws = [0, 1, ONE - 1, ONE, ONE + 1, (1 << 53) - 2, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3,
          (1 << 54) - 1, (1 << 54) + 1, (1 << 54) + 3, (1 << 60) + 12345, (1 << 62) - 1, F - 1, MAX_SAMPLES * ONE, MAX_SAMPLES * ONE - 1]
    ws += [int(x) for x in rng.integers(0, n * ONE, 96, dtype=np.uint64, endpoint=True)]
    # either side of every exact byte boundary (the smallest sum whose mean reaches it: bisection's answer, in closed form)
    for b in BOUNDS:
        c = math.ceil(b * ONE * n)
        ws += [c - 1, c]
    # either side of where the implementation's byte actually flips: bisection on the integer sum (the byte is monotone in it)
    c = [math.ceil(b * ONE * n) for b in BOUNDS]
    lo = np.array([x - (x >> 18) - 1 for x in c], np.uint64)   # the byte's error is far below 2^-18 (relative) of the sum
    hi = np.array([x + (x >> 18) + 1 for x in c], np.uint64)
    k = np.arange(1, 256)
    assert (resolve_lib(np.repeat(lo, 3), n, want_lin=False)[0][::3] < k).all() and (resolve_lib(np.repeat(hi, 3), n, want_lin=False)[0][::3] >= k).all()
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // np.uint64(2)
        rgb, _ = resolve_lib(np.repeat(mid, 3), n, want_lin=False)
        up = rgb[::3] >= k
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    ws += [int(x) for x in hi] + [int(x) - 1 for x in hi]
    # f32 rounding midpoints of the mean: where the f64 chain's own rounding can decide the f32 (large sums, above 2^53)
    for m_bits in (0x3E800001, 0x3F000001, 0x3F400001, 0x3F7FFFFF, 0x3C000003):
        lo_f = np.array(m_bits, np.uint32).view(np.float32)
        m = (Fraction(float(lo_f)) + Fraction(float(np.nextafter(lo_f, np.float32(2))))) / 2
        s0 = round(m * ONE * n)
        step = max(1, (1 << max(0, s0.bit_length() - 53)) // 8)
        ws += [s0 + j * step for j in range(-24, 25) if 0 <= s0 + j * step < F]
    # flagged words: bit 63 over arbitrary low bits
    ws += [F | x for x in (0, 1, ONE, n * ONE, F - 1, int(rng.integers(0, F)))]
    ws += [0] * (-len(ws) % 3)
    return np.array(ws, np.uint64)


@pytest.fixture(scope="module")
def crafted(resolve_lib):
    return {n: _crafted_words(n, resolve_lib) for n in NS}


# ---------------------------------------------------------------------------------------------------- no GPU needed

@pytest.mark.parametrize("name,w,h,n,depth", [("cover", 20, 14, 12, 50), ("test", 20, 14, 12, 8)])
def test_oracle_accumulate_equals_oracle_render(oracle, abi, load_scene, name, w, h, n, depth):
    """[0, N) accumulated and resolved exactly is the oracle's one-shot frame at N samples, within the pooled bar; same paths"""
    sc = load_scene(name, w, h, n, depth=depth)
    acc, st = oracle.accumulate(abi, sc.ptr, 0, n)
    o_rgb, o_lin, o_st = oracle.render(abi, sc.ptr)
    assert not (acc & np.uint64(F)).any()
    lin = np.array([float(_f32_rn(Fraction(int(x), ONE * n))) for x in acc.ravel()], np.float32).reshape(acc.shape)
    rgb = _f32_to_u8(np.sqrt(lin))
    assert_parity(rgb, lin, o_rgb, o_lin, f"oracle accumulate {name} [0, {n})", atol=pooled_atol(n))
    for k in ("segments", "segments_discarded", "tex_oob", "samples"):
        assert st[k] == o_st[k], (k, st[k], o_st[k])


def test_oracle_accumulate_splits(oracle, abi, load_scene):
    """any split of [0, N), in any order, into one accumulator gives the same words; other pixels are left alone"""
    sc = load_scene("test", 16, 10, 12, depth=8)
    whole, st = oracle.accumulate(abi, sc.ptr, 0, 12)
    for split in ([(0, 1), (1, 12)], [(7, 12), (0, 3), (3, 7)], [(s, s + 1) for s in range(11, -1, -1)]):
        acc = None
        segs = 0
        for b, e in split:
            acc, s = oracle.accumulate(abi, sc.ptr, b, e - b, accum=acc)
            segs += s["segments"]
        assert np.array_equal(acc, whole), split
        assert segs == st["segments"], split
    # a window and row tiles address the same words
    t = abi.RtRowTiles(2, 1, 3)
    rows = abi.tiles_global_rows(sc.c.height, t)
    acc, _ = oracle.accumulate(abi, sc.ptr, 0, 12, tiles=t, x_range=(3, 11))
    assert np.array_equal(acc[:, 3:11], whole[rows, 3:11]) and not acc[:, :3].any() and not acc[:, 11:].any()


def test_f32_to_u8_restatement(oracle, abi):
    L = oracle.lib(abi)
    x = np.concatenate([np.linspace(-0.01, 1.01, 20001, dtype=np.float32), np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0]),
                        (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)])
    assert np.array_equal(_f32_to_u8(x), np.array([L.rt_oracle_f32_to_u8(float(v)) for v in x], np.uint8))


def test_resolve_against_exact_arithmetic(oracle, abi, resolve_lib, crafted):
    """hostsim_resolve (rt_core.h fixed_to_mean, rt_nanf, f32_to_u8 of sqrtf) on the crafted words against exact rationals.

    The mean is computed as f32(f64(f64(sum) * 2^-40) / n): f64(sum) rounds when sum > 2^53, the division rounds, then the
    f32 conversion rounds.  Each f64 step has a relative error of at most 2^-53, so the f64 value d is within 2^-52 (relative)
    of the exact mean q, and the f32 result can differ from q rounded to f32 only if an f32 rounding midpoint lies between q
    and d (inclusive): double rounding.  Then it is the other neighbour of that midpoint, 1 ulp away.  Every mismatch must be
    such a case; the words crafted around f32 midpoints at large n make some happen.

    The byte: sqrtf and the f32 product x * 255 each add at most half an ulp (relative 2^-24) to the 1 ulp of the mean, in all
    about 1.5 * 2^-22 relative in mean terms.  So the byte equals the exact rational byte round(255 sqrt(q)) unless q lies
    within 2^-20 (relative) of a boundary ((k - 0.5) / 255)^2, and is within 1 of it always."""
    L = oracle.lib(abi)
    mismatches = near = 0
    for n in NS:
        words = crafted[n]
        rgb, lin = resolve_lib(words, n)
        flagged = (words & np.uint64(F)) != 0
        assert np.isnan(lin[flagged]).all() and (rgb[flagged] == 255).all(), n
        for w, l, r in zip(words[~flagged].tolist(), lin[~flagged], rgb[~flagged]):
            q = Fraction(w, ONE * n)
            d = (float(w) * 2.0 ** -40) / n
            assert l == np.float32(d), (n, w)                       # the f64 chain as restated in the docstring
            assert abs(Fraction(d) - q) <= q * Fraction(1, 2 ** 52), (n, w)
            assert abs(Fraction(float(l)) - q) <= Fraction(float(np.spacing(l))), (n, w, l)   # within 1 ulp of the exact mean
            cr = _f32_rn(q)
            if l != cr:
                mismatches += 1
                mid = (Fraction(float(l)) + Fraction(float(cr))) / 2
                assert min(q, Fraction(d)) <= mid <= max(q, Fraction(d)), f"n {n} sum {w}: {l!r} is not q rounded ({cr!r}) and no double rounding explains it"
            assert r == L.rt_oracle_f32_to_u8(float(np.sqrt(np.float32(l)))), (n, w)
            eb = _exact_byte(q)
            assert abs(int(r) - eb) <= 1, (n, w, r, eb)
            if any(abs(q - b) <= b * Fraction(1, 2 ** 20) for b in BOUNDS[max(0, eb - 2):eb + 2]):
                near += 1
            else:
                assert r == eb, f"n {n} sum {w}: byte {r}, exact {eb}, and no boundary is near"
    assert mismatches > 0, "no word reached the double rounding of sums above 2^53"
    assert near > 0


# ---------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _to_dev(torch, words):
    return torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64)).to("cuda:0")


def _words(acc):
    return acc.cpu().numpy().view(np.uint64)


def _check_words(got, want, count, what):
    """a GPU accumulator against the oracle's: flags identical, sums within LINEAR_ATOL on the mean"""
    assert got.shape == want.shape, what
    fl = np.uint64(F)
    assert np.array_equal(got & fl, want & fl), f"{what}: NaN flags differ"
    d = np.abs((got & ~fl).astype(np.int64) - (want & ~fl).astype(np.int64)).max()
    assert d <= count * ONE * LINEAR_ATOL, f"{what}: max |sum difference| {d} = {d / count / ONE:.3g} on the mean"


HIGH_SCENES = {   # name -> (scene, width, height, depth, options)
    "cover": ("cover", 64, 48, 50, ()),
    "lit": ("test", 48, 36, 8, ()),
    "lit_pools32": ("test", 48, 36, 8, (("light_pool", 32), ("light_base_pool", 32))),
}


@pytest.fixture(scope="module")
def oracle_ranges(oracle, abi, load_scene):
    """oracle.accumulate of a range of a HIGH_SCENES scene (its options shape the GPU's work only: the lit configurations share one)"""
    cache = {}

    def get(config, b, e):
        name, w, h, depth, _ = HIGH_SCENES[config]
        key = (name, w, h, depth, b, e)
        if key not in cache:
            sc = load_scene(name, w, h, 1, depth=depth)
            cache[key] = oracle.accumulate(abi, sc.ptr, b, e - b)
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(HIGH_SCENES))
def test_high_sample_indices_against_oracle(pkg, abi, oracle_ranges, torch_cuda, load_scene, config):
    """sample ranges up to 2^23 - 2, automatic chunks and 5-sample chunks (multi-chunk items at a non-zero base), word for word
    against the oracle's accumulate at the same indices"""
    torch = torch_cuda
    name, w, h, depth, opts = HIGH_SCENES[config]
    sc = load_scene(name, w, h, 1, depth=depth)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    for k, v in opts:
        gs.set_option(k, v)
    frames = {}
    for chunk in (0, 5):
        gs.set_option("chunk_spp", chunk)
        for b, e in RANGES + ((5, 29),):
            what = f"{config} [{b}, {e}) chunk_spp {chunk}"
            acc = _new_accum(torch, gs)
            st = _accumulate(torch, gs, acc, [(b, e)])
            rgb, lin = _resolve(torch, gs, acc, e - b)
            frames[(chunk, b)] = lin
            if (b, e) == (5, 29):
                continue
            want, ost = oracle_ranges(config, b, e)
            _check_words(_words(acc), want, e - b, what)
            assert st["segments"] == ost["segments"] - ost["segments_discarded"], (what, st["segments"], ost)
            assert st["tex_oob"] == ost["tex_oob"], (what, st["tex_oob"], ost["tex_oob"])
            o_rgb, o_lin = _resolve_ref(want.ravel(), e - b)
            assert_parity(rgb, lin, o_rgb.reshape(rgb.shape), o_lin.reshape(lin.shape), what, atol=LINEAR_ATOL)
        # a kernel that ignored the base would render [5, 29) for [2^20 + 5, 2^20 + 29)
        hi = frames[(chunk, (1 << 20) + 5)]
        differ = (hi != frames[(chunk, 5)]).any(axis=2).mean()
        assert differ > 0.5, f"{config}: the [2^20 + 5, +24) frame equals the [5, 29) frame at {1 - differ:.0%} of the pixels"
    gs.close()


SATURATED = {"width": 8, "height": 6, "samples_per_pixel": 1, "max_depth": 8, "sky": None,
             "camera": {"look_from": {"x": 0.0, "y": 0.0, "z": 0.0}, "look_at": {"x": 0.0, "y": 0.0, "z": -1.0},
                        "vup": {"x": 0.0, "y": 1.0, "z": 0.0}, "vfov": 90.0, "aspect": 1.3333333333333333},
             "objects": [{"center": {"x": 0.0, "y": 0.0, "z": 0.0}, "radius": 10.0, "material": {"Light": {}}}]}


@pytest.mark.gpu
def test_accumulator_at_its_limit(pkg, abi, oracle, host, torch_cuda):
    """a world whose every sample is exactly 1.0 (the camera inside a Light sphere: materials.rs:65-69 returns the light's
    (1, 1, 1)) fills words prefilled with (2^23 - 4) samples to exactly (2^23 - 1) * 2^40 — no carry into the flag"""
    torch = torch_cuda
    sc = host.Scene.loads(json.dumps(SATURATED))
    b, e = MAX_SAMPLES - 3, MAX_SAMPLES
    ref, _ = oracle.accumulate(abi, sc.ptr, b, e - b)
    assert (ref == np.uint64(3 * ONE)).all(), "the saturated world's samples are not all exactly 1.0"
    shape = ref.shape
    rng = np.random.default_rng(7)
    flag = rng.random(shape) < 0.3
    pre = np.full(shape, (MAX_SAMPLES - 3) * ONE, np.uint64) | np.where(flag, np.uint64(F), np.uint64(0))
    gs = pkg.hip.HipScene(sc.ptr, 0)
    acc = _to_dev(torch, pre)
    _accumulate(torch, gs, acc, [(b, e)])
    got = _words(acc)
    want = np.uint64(0x7FFFFF0000000000) | np.where(flag, np.uint64(F), np.uint64(0))
    assert np.array_equal(got, want), f"{int((got != want).sum())} words are not (2^23 - 1) * 2^40 (+ their flag)"
    rgb, lin = _resolve(torch, gs, acc, MAX_SAMPLES)
    assert (lin[~flag] == 1.0).all() and np.isnan(lin[flag]).all() and (rgb == 255).all()
    with pytest.raises(pkg.host.RtError) as err:
        gs.accumulate(acc.data_ptr(), MAX_SAMPLES, 1, stream=_stream(torch))
    assert err.value.code == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(_words(acc), want), "a refused pass changed the accumulator"
    gs.close()


@pytest.mark.gpu
def test_accumulate_adds_to_a_callers_words(pkg, abi, oracle, torch_cuda, load_scene):
    """prefilled words whose low dwords are within 256 of a carry (and some NaN flags): each must become prefill + the pass's
    sums — a lost carry between the dwords or an overwrite instead of an add fails"""
    torch = torch_cuda
    sc = load_scene("cover", 32, 24, 1, depth=50)
    b, e = (1 << 22) + 7, (1 << 22) + 15
    ref, _ = oracle.accumulate(abi, sc.ptr, b, e - b)
    rng = np.random.default_rng(11)
    low = rng.integers(0xFFFFFF00, 0xFFFFFFFF, ref.shape, dtype=np.uint64, endpoint=True)
    high = rng.integers(0, 1 << 30, ref.shape, dtype=np.uint64) << np.uint64(32)
    flag = np.where(rng.random(ref.shape) < 0.2, np.uint64(F), np.uint64(0))
    pre = high | low | flag
    gs = pkg.hip.HipScene(sc.ptr, 0)
    acc = _to_dev(torch, pre)
    _accumulate(torch, gs, acc, [(b, e)])
    got = _words(acc)
    assert np.array_equal(got & np.uint64(F), flag | (ref & np.uint64(F))), "NaN flags of the prefill were lost or invented"
    _check_words(got & ~np.uint64(F), (pre & ~np.uint64(F)) + ref, e - b, "prefill + [2^22 + 7, 2^22 + 15)")
    gs.close()


def _resolve_into(torch, gs, acc_dev, n, n_px, off, want_rgb, want_lin, tiles):
    """rt_resolve with d_rgb8 at byte offset `off` inside a sentinel-filled buffer (16 guard bytes either side) and d_linear
    between guard floats; -> (rgb bytes, guards intact?, linear, guards intact?)"""
    g = 16
    buf = torch.full((n_px * 3 + 2 * g + 4,), 0xA5, dtype=torch.uint8, device="cuda:0")
    lbuf = torch.full((n_px * 3 + 8,), -7.0, dtype=torch.float32, device="cuda:0")
    gs.resolve(acc_dev.data_ptr(), n, buf.data_ptr() + g + off if want_rgb else 0, lbuf.data_ptr() + 16 if want_lin else 0, tiles, _stream(torch))
    torch.cuda.current_stream().synchronize()
    hb, hl = buf.cpu().numpy(), lbuf.cpu().numpy()
    body = hb[g + off:g + off + n_px * 3]
    rest = np.concatenate([hb[:g + off], hb[g + off + n_px * 3:]]) if want_rgb else hb
    lrest = np.concatenate([hl[:4], hl[4 + n_px * 3:]]) if want_lin else hl
    return body, bool((rest == 0xA5).all()), hl[4:4 + n_px * 3], bool((lrest == -7.0).all())


def _resolve_all_ways(torch, gs, words, n, tiles, want_rgb, want_lin, what):
    n_px = words.size // 3
    acc = _to_dev(torch, words)
    for off in range(4):
        rgb, rgb_guard, lin, lin_guard = _resolve_into(torch, gs, acc, n, n_px, off, True, True, tiles)
        assert rgb_guard and lin_guard, f"{what} offset {off}: a guard byte or float was written"
        assert np.array_equal(rgb, want_rgb), f"{what} offset {off}: RGB8 differs at {int((rgb != want_rgb).sum())} of {rgb.size}"
        assert np.array_equal(lin.view(np.uint32), want_lin.view(np.uint32)), f"{what} offset {off}: linear differs bitwise"
        rgb1, g1, _, lg1 = _resolve_into(torch, gs, acc, n, n_px, off, True, False, tiles)
        assert g1 and lg1 and np.array_equal(rgb1, want_rgb), f"{what} offset {off}: the RGB8-only resolve differs"
    _, g2, lin2, lg2 = _resolve_into(torch, gs, acc, n, n_px, 0, False, True, tiles)
    assert g2 and lg2 and np.array_equal(lin2.view(np.uint32), want_lin.view(np.uint32)), f"{what}: the linear-only resolve differs"


@pytest.mark.gpu
def test_resolve_kernel_matches_hostsim_bit_for_bit(pkg, abi, torch_cuda, load_scene, resolve_lib, crafted):
    """rt_resolve on the crafted words: every n, RGB8 at byte offsets 0-3 (dword and byte stores), linear only, RGB8 only, odd
    pixel counts and row tiles; the bytes around the outputs stay untouched"""
    torch = torch_cuda
    # the whole word set of each n through a 7 x H frame (H odd: 7H = 3 mod 4 pixels, a byte-stored tail)
    most = max(c.size for c in crafted.values()) // 3
    h = -(-most // 7) | 1
    sc = load_scene("cover", 7, h, 1)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    for n in NS:
        words = np.resize(crafted[n], 7 * h * 3)
        rgb, lin = resolve_lib(words, n)
        _resolve_all_ways(torch, gs, words, n, None, rgb, lin, f"7x{h} n {n}")
    gs.close()
    # small frames (n_px mod 4 = 1, 3, 3, 3, 2), whole and as row tiles {2, r, 3}
    for w, hh in ((1, 1), (3, 1), (7, 5), (13, 11), (2, 3)):
        sc = load_scene("cover", w, hh, 1)
        gs = pkg.hip.HipScene(sc.ptr, 0)
        for tiles in (None, abi.RtRowTiles(2, 0, 3), abi.RtRowTiles(2, 1, 3), abi.RtRowTiles(2, 2, 3)):
            n_px = abi.tiles_local_rows(hh, tiles) * w
            if n_px == 0:
                continue
            for i, n in enumerate((1, 3, 8191, MAX_SAMPLES)):
                words = np.roll(crafted[n], -97 * (w + hh + i))[:n_px * 3]
                rgb, lin = resolve_lib(words, n)
                _resolve_all_ways(torch, gs, words, n, tiles, rgb, lin, f"{w}x{hh} tiles {tiles and (tiles.tile_rows, tiles.first_tile, tiles.tile_stride)} n {n}")
        gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(7, 5), (13, 11)])
def test_odd_pixel_counts_end_to_end(pkg, torch_cuda, load_scene, w, h):
    torch = torch_cuda
    sc = load_scene("cover", w, h, 8)
    _split_equals_one_shot(torch, pkg, sc, [(0, 3), (3, 8)], what=f"cover {w}x{h}")
    gs = pkg.hip.HipScene(sc.ptr, 0)
    ps = pkg.hip.HipScene(sc.ptr, 0)
    for k, n in ((3, 3), (5, 8)):
        img, _ = ps.refine_to_host(k)
        gs.set_option("samples_per_pixel", n)
        want, _ = gs.render_to_host()
        assert np.array_equal(img, want), (w, h, n)
    gs.close(); ps.close()


@pytest.mark.gpu
def test_cli_passes_odd_pixel_count(pkg, torch_cuda, tmp_path):
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "cfg2_cover_1200x800_spp128.json")))
    cfg.update(width=13, height=11, samples_per_pixel=8)
    path = tmp_path / "odd.json"
    path.write_text(json.dumps(cfg))
    one, prog = str(tmp_path / "one.png"), str(tmp_path / "prog.png")
    r1 = _cli([str(path), one])
    r3 = _cli([str(path), prog, "--passes", "3"])
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr, r3.stderr)
    assert open(one, "rb").read() == open(prog, "rb").read(), "13x11: the last pass's PNG is not the one-shot PNG"


# every option that does not restart the scene's accumulator, set to other accepted values before each pass
OPTION_STEPS = (
    {"tile_log2": 1, "tile_shape": 1, "tile_order": 0, "tile_affinity": 2, "tile_batch": 1, "chunk_spp": 2, "variant": 1,
     "light_pool": 32, "light_base_pool": 32, "light_nest_pool": 0, "force_lit": 1, "samples_per_pixel": 3},
    {"tile_log2": 3, "tile_shape": 3, "tile_order": 1, "tile_affinity": 0, "tile_batch": 64, "chunk_spp": 1, "variant": 0,
     "light_pool": 1024, "light_base_pool": 64, "light_nest_pool": 1, "force_lit": 0, "samples_per_pixel": 1000},
    {"tile_log2": 0, "tile_shape": 2, "tile_order": 2, "tile_affinity": 1, "tile_batch": 7, "chunk_spp": 0, "variant": 1,
     "light_pool": 0, "light_base_pool": 0, "light_nest_pool": 0, "force_lit": 1, "samples_per_pixel": 0},
)
OPTION_PASSES = (3, 6, 2, 5)   # 16 samples


@pytest.mark.gpu
def test_options_between_passes(pkg, abi, torch_cuda, load_scene):
    torch = torch_cuda
    sc = load_scene("test", 48, 36, 16, depth=8)
    gs = pkg.hip.HipScene(sc.ptr, 0)
    want, _ = gs.render_to_host()
    one = _one_shot(torch, gs, 16, abi=abi)
    gs.close()
    ps = pkg.hip.HipScene(sc.ptr, 0)
    n = 0
    for i, k in enumerate(OPTION_PASSES):
        if i:
            for key, v in OPTION_STEPS[i - 1].items():
                ps.set_option(key, v)
        img, _ = ps.refine_to_host(k)
        n += k
        assert ps.query("accum_samples") == n, (i, ps.query("accum_samples"), n)
    assert np.array_equal(img, want), f"refine_to_host with options changed between passes: {int((img != want).sum())} values differ"
    ps.close()
    ps = pkg.hip.HipScene(sc.ptr, 0)
    acc = _new_accum(torch, ps)
    b = 0
    for i, k in enumerate(OPTION_PASSES):
        if i:
            for key, v in OPTION_STEPS[i - 1].items():
                ps.set_option(key, v)
        _accumulate(torch, ps, acc, [(b, b + k)])
        b += k
    _assert_identical(_resolve(torch, ps, acc, 16), one, "accumulate with options changed between passes")
    ps.close()
