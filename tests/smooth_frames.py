"""The restatement's frames of the parity cases of shading normals, computed once per session and left unchanged: the CPU and
the GPU tests share them.  TEST INFRASTRUCTURE."""
import smooth_mini as SMM
import smooth_worlds as SW
from test_medium_gpu import _load

DEPTH = 8
_CACHE = {}


def world(host, case):
    """(host scene, center1, lens, quads, normals [n, 9]) of one parity case: 48 x 32 at spp 4"""
    sc, c1, lens = _load(host, SW.parity_cfg(case), SW.W, SW.H, SW.SPP, DEPTH, seed=97)
    n = sc.flat_normals()
    assert n is not None and (c1 is not None) == ("moving" in case) and (lens is not None) == ("lens" in case)
    return sc, c1, lens, sc.quads(), n


def mini(oracle, abi, sc, c1, lens, quads, normals):
    L = oracle.lib(abi)
    return SMM.SmoothMini(sc.c, lambda y, x: L.rt_oracle_atan2(y, x), c1, lens, quads, normals)


def mini_frame(oracle, abi, host, case):
    if case not in _CACHE:
        sc, c1, lens, quads, normals = world(host, case)
        m = mini(oracle, abi, sc, c1, lens, quads, normals)
        rgb, lin, segs = m.render()
        rgb.setflags(write=False); lin.setflags(write=False)
        _CACHE[case] = {"rgb": rgb, "lin": lin, "segments": segs, "discarded": m.discarded, "shaded": m.shaded, "fell": dict(m.fell)}
    return _CACHE[case]
