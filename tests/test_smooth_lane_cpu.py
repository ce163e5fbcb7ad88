"""The CPU build of the QUADS lane code with shading normals (tests/smoothsim/lane_smooth.cpp over tests/lanesim/lane_sim.h):
object_surface<true> with FLAT_NORMALS_BIT — the header's pointer, the entry-order index, the call — without a GPU.  The GPU test's
frames against SmoothMini at tests/parity.py's bar with exact segment counts (Lambertian, Metal, Glass, Checker), AOV normals bitwise, the
structure against the scan bit for bit, and the checks that need no restatement: the axis-aligned identity and set / remove."""
import numpy as np
import pytest

import lane_smooth
import smooth_frames as SF
import smooth_mini as SMM
import smooth_worlds as SW
from parity import assert_parity, pooled_atol
from test_medium_gpu import _load

W, H, SPP = SW.W, SW.H, SW.SPP


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    assert a[0] == b[0] == 0, what
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2])) and a[3] == b[3] > 0, what


@pytest.mark.parametrize("case", SW.PINHOLE_CASES)
def test_lane_code_against_the_restatement(abi, oracle, host, case):
    """the frame of the lane code with normals: SmoothMini's at the parity bar, its segments exactly; not the frame without normals; the
    structure gives the scan's frame bit for bit (the records are indexed by entry, not in BVH order); the AOVs are SmoothMini's in every bit"""
    L = lane_smooth.load(abi)
    sc, c1, lens, quads, normals = SF.world(host, case)
    assert c1 is None and lens is None
    got = L.render(sc.c, quads, normals)
    rc, rgb, lin, segs, info = got
    n_smooth = len(quads) - 2
    assert rc == 0 and info[0] & lane_smooth.FLAT_NORMALS_BIT and not info[0] & lane_smooth.FLAT_BVH_BIT and info[1] == n_smooth == (320 if case == "metal" else 80)
    m = SF.mini_frame(oracle, abi, host, case)
    print(f"{case}: max |linear diff| {float(np.abs(lin - m['lin']).max()):.3g}, segments lane {segs} mini {m['segments']} - {m['discarded']}, fell {m['fell']}")
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(SPP))
    assert segs == m["segments"] - m["discarded"]
    flat = L.render(sc.c, quads, None)
    assert flat[0] == 0 and not flat[4][0] & lane_smooth.FLAT_NORMALS_BIT and not np.array_equal(_bits(flat[2]), _bits(lin))
    bvh = L.render(sc.c, quads, normals, flat_bvh=True)
    assert bvh[4][0] & lane_smooth.FLAT_BVH_BIT and bvh[4][0] & lane_smooth.FLAT_NORMALS_BIT
    _same(bvh, got, case + ": the structure")
    rc, aov = L.aovs(sc.c, quads, SPP, normals)
    want = SF.mini(oracle, abi, sc, c1, lens, quads, normals).aovs(SPP)
    assert rc == 0 and np.array_equal(_bits(aov), _bits(want)), float(np.abs(aov - want).max())
    rc, aov_bvh = L.aovs(sc.c, quads, SPP, normals, flat_bvh=True)
    assert rc == 0 and np.array_equal(_bits(aov_bvh), _bits(aov))
    rc, aov_flat = L.aovs(sc.c, quads, SPP, None)
    assert rc == 0 and not np.array_equal(_bits(aov_flat[:, :, 4:7]), _bits(aov[:, :, 4:7]))


def test_axis_aligned_identity(abi, host):
    """a box of 12 triangles, each carrying its face's axis as all three normals: s is exactly the axis, and the frame and the AOVs are
    those of ANOTHER scene, without normals, bit for bit"""
    L = lane_smooth.load(abi)
    out = {}
    for with_normals in (True, False):
        sc, _, _ = _load(host, SW.box_cfg(with_normals), W, H, SPP, 8, seed=5)
        n = sc.flat_normals()
        assert (n is not None) == with_normals
        out[with_normals] = (L.render(sc.c, sc.quads(), n), L.aovs(sc.c, sc.quads(), SPP, n))
    assert out[True][0][4][1] == 12 and out[True][0][4][0] & lane_smooth.FLAT_NORMALS_BIT and not out[False][0][4][0] & lane_smooth.FLAT_NORMALS_BIT
    _same(out[True][0], out[False][0], "axis-aligned normals")
    assert np.array_equal(_bits(out[True][1][1]), _bits(out[False][1][1]))


def test_set_and_remove_and_refusals(abi, host):
    """nine zeros on every entry is a scene that never had normals (no bit, the same frame); a refused vector and a parallelogram with
    normals name the lowest bad entry"""
    L = lane_smooth.load(abi)
    sc, c1, lens, quads, normals = SF.world(host, "glass")
    never = L.render(sc.c, quads, None)
    zeros = L.render(sc.c, quads, np.zeros_like(normals))
    assert zeros[4][:2] == never[4][:2] and not zeros[4][0] & lane_smooth.FLAT_NORMALS_BIT
    _same(zeros, never, "nine zeros everywhere")
    for bvh in (False, True):
        _same(L.render(sc.c, quads, np.zeros_like(normals), flat_bvh=bvh), L.render(sc.c, quads, None, flat_bvh=bvh), "removed")
    assert quads[0].reserved == abi.RT_QUAD_SHAPE_PARALLELOGRAM
    bad = normals.copy(); bad[50, 4] = np.nan; bad[30, 0:3] = 0.0
    assert L.render(sc.c, quads, bad)[0] == 2 and L.render(sc.c, quads, bad)[4][2] == 30
    bad = normals.copy(); bad[1, 2] = 1.0; bad[30, 0:3] = 0.0
    assert L.render(sc.c, quads, bad)[4][2] == 1
