"""The order table of the flat-primitive BVH as the device build makes it, without a GPU: the RT_HD expressions of
rt_flat_build.h — centre, range by count, ordered bits, axis choice, comparator, leaf order — compiled by g++ and driven step by step as
rt_flat_build.hip build() enqueues its kernels (tests/flatbuild/flat_build_emu.cpp: a loop per kernel, std::sort for the device's sort),
against the builder restated in Python from the contract (tests/flat_build_worlds.py) and against the host builder's own order table
(tests/flat_bvh_sim.py: rt_tables.h build_flat_bvh).  Equality of whole tables; no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flat_build_worlds as B
import flat_bvh_sim as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "hip")
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = tmp_path_factory.mktemp("flat_build_emu") / "libflat_build_emu.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "flatbuild", "flat_build_emu.cpp"), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    P, u32 = C.c_void_p, C.c_uint32
    L.fbd_build.argtypes = [P, P, P, u32, P, P, P]
    L.fbd_ordered_bits.argtypes = [P, u32, P, P]
    L.fbd_ordered_bits.restype = None
    return L


def _emulated(emu, ok, lo, hi):
    """-> order, boxed entries, depths, axes per depth (bit masks)"""
    ok = np.ascontiguousarray(ok, np.int32)
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    n = len(ok)
    order, info, axes = np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(2, np.uint32), np.zeros(32, np.uint32)
    assert emu.fbd_build(lo.ctypes.data, hi.ctypes.data, ok.ctypes.data, n, order.ctypes.data, info.ctypes.data, axes.ctypes.data) == 0
    return order, int(info[0]), int(info[1]), axes[:int(info[1])].tolist()


def _world_boxes(abi, name):
    sim = F.load(abi)
    flats = F.flats_array(abi, B.world(name), 1)
    ok, lo, hi = sim.entry_boxes(flats)
    _, order, n_always = sim.build(flats)
    lo[~ok], hi[~ok] = 0.0, 0.0             # (a refused entry's box is never read)
    return ok, lo, hi, order, n_always


WORLDS = ["n%d" % n for n in B.SIZES] + ["equal", "zeros", "axes", "needles1", "needles4", "needles5"]


@pytest.mark.parametrize("name", WORLDS)
def test_emulated_device_build_equals_the_contract_and_the_host_builder(emu, abi, name):
    ok, lo, hi, host_order, n_always = _world_boxes(abi, name)
    got, m, depths, axes = _emulated(emu, ok, lo, hi)
    seen = {}
    want = B.python_order(ok, lo, hi, seen)
    assert m == int(ok.sum()) == len(ok) - n_always and depths == B.depths(m) == len(seen)
    assert np.array_equal(got, want), name
    assert np.array_equal(got, host_order), name
    assert axes == [sum(1 << a for a in seen[d]) for d in range(depths)]
    if name[0] == "n" and name[1:].isdigit():
        assert n_always == 0 and m == int(name[1:])
    if name in B.NEEDLES:
        assert n_always == len(B.NEEDLES[name]) and got[:n_always].tolist() == B.NEEDLES[name]
    if name == "axes":
        assert depths == 3 and axes[:2] == [1, 1] and axes[2] == 0b111      # three axes at one depth
    if name == "equal":
        assert got.tolist() == list(range(37))                             # every split by index alone: the order table is the identity
    if name == "zeros":
        c = 0.5 * lo[:, 0] + 0.5 * hi[:, 0]
        assert (c == 0.0).sum() == 14 and (c > 0.0).sum() == 14 and (c < 0.0).sum() == 13 and axes == [1] * depths


def test_depths_and_ranges_follow_from_the_count(emu):
    """1, 4: no depth; 5, 8: one; 9: two; 1025: nine; 4099: eleven; 2^16 + 3: fifteen; 2^18: sixteen"""
    assert [B.depths(m) for m in (0, 1, 4, 5, 8, 9, 1025, 4099, 65539, 2 ** 18)] == [0, 0, 0, 1, 1, 2, 9, 11, 15, 16]
    for m in (5, 9, 1025, 4099):
        got = _emulated(emu, np.ones(m, np.int32), np.zeros((m, 3)), np.ones((m, 3)))
        assert got[2] == B.depths(m) and got[0].tolist() == list(range(m))


def test_signed_zero_centres_tie_and_fall_to_the_index(emu):
    """boxes whose centres are -0.0 and +0.0 (lo = hi = the zero itself; no padded box has such a centre, so this world exists on the
    host only): they compare equal and the index decides — a sort on raw bit patterns would put every -0.0 first"""
    rng = np.random.default_rng(8)
    n = 45
    x = np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0)
    x[::9] = [-1.0, 1.0, -2.0 ** -1074, 2.0 ** -1074, 3.0]
    assert np.signbit(x[x == 0.0]).any() and not np.signbit(x[x == 0.0]).all()
    lo = np.zeros((n, 3))
    lo[:, 0] = x
    ok = np.ones(n, np.int32)
    got, m, depths, axes = _emulated(emu, ok, lo, lo.copy())
    want = B.python_order(ok, lo, lo)
    assert np.array_equal(got, want) and axes == [1] * depths
    by_bits = np.lexsort((np.arange(n), lo[:, 0].view(np.int64)))
    assert not np.array_equal(np.sort(want[: n // 2]), np.sort(by_bits[: n // 2]))   # (the world does tell the two orders apart)


def test_ordered_bits_keep_the_order_of_doubles(emu):
    x = np.array([-np.inf, -1e300, -1.0, -2.0 ** -1074, -0.0, 0.0, 2.0 ** -1074, 1.0, 1.5, 1e300, np.inf])
    bits, back = np.zeros(len(x), np.uint64), np.zeros(len(x))
    emu.fbd_ordered_bits(x.ctypes.data, len(x), bits.ctypes.data, back.ctypes.data)
    assert (np.diff(bits.astype(object)) > 0).all()
    assert np.array_equal(back.view(np.uint64), x.view(np.uint64))


def test_the_host_builder_runs_the_shared_expressions():
    """rt_tables.h build_flat_bvh calls the RT_HD functions the device build calls: one definition of the split"""
    tables = open(os.path.join(HIP_DIR, "rt_tables.h")).read()
    shared = open(os.path.join(HIP_DIR, "rt_flat_build.h")).read()
    device = open(os.path.join(HIP_DIR, "rt_flat_build.hip")).read()
    for f in ("flat_centre(", "flat_split_axis(", "flat_split_less("):
        assert f in tables and "RT_HD" in shared[shared.index(f) - 40:shared.index(f)], f
    for f in ("flat_centre(", "flat_split_axis(", "flat_item_less(", "flat_range_at(", "flat_leaf_sort(", "flat_ordered_bits("):
        assert f in device, f


def test_cli_flat_rebuild_flag_parsing(pkg, tmp_path):
    """--flat-rebuild K: only with --flat-frames, K >= 1, once; a refused command line prints the usage line, an accepted one goes on to
    read the scene file, which does not exist here"""
    exe = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
    cases = [
        (["--flat-rebuild", "2"], True),
        (["--frames", "3", "--flat-rebuild", "2"], True),
        (["--frames", "3", "--flat-frames", "p_", "--flat-rebuild"], True),
        (["--frames", "3", "--flat-frames", "p_", "--flat-rebuild", "0"], True),
        (["--frames", "3", "--flat-frames", "p_", "--flat-rebuild", "-1"], True),
        (["--frames", "3", "--flat-frames", "p_", "--flat-rebuild", "x"], True),
        (["--frames", "3", "--flat-frames", "p_", "--flat-rebuild", "2", "--flat-rebuild", "3"], True),
        (["--frames", "3", "--flat-frames", "p_", "--flat-rebuild", "2"], False),
        (["--flat-rebuild", "1", "--frames", "3", "--orbit", "0", "--flat-frames", "p_", "--flat-bvh"], False),
    ]
    for args, usage in cases:
        r = subprocess.run([exe, str(tmp_path / "missing.json"), str(tmp_path / "out")] + args, capture_output=True, text=True, timeout=60)
        if usage:
            assert r.returncode == 0 and r.stdout.startswith("Usage:"), (args, r.returncode, r.stdout, r.stderr)
        else:
            assert r.returncode == 101 and "Unable to read config file" in r.stderr and "Usage" not in r.stdout, (args, r.returncode, r.stdout, r.stderr)
