"""tests/smoothsim/lane_smooth.cpp (the CPU build of the QUADS lane code with shading normals; a g++ build with
-ffp-contract=off): load(abi) builds it once per session and returns numpy wrappers around its entry points."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT_BVH_BIT, FLAT_NORMALS_BIT = 0x80000000, 0x40000000
_loaded = None


class LaneSmooth:
    def __init__(self, L, abi):
        self.L = L
        S, P, u32 = C.POINTER(abi.RtScene), C.c_void_p, C.c_uint32
        L.lane_smooth_render.argtypes = [S, P, P, u32, P, C.c_int, P, P, P, P]
        L.lane_smooth_aovs.argtypes = [S, P, P, u32, P, C.c_int, u32, P]

    @staticmethod
    def _args(sc, center1, quads, normals):
        s = sc.contents if hasattr(sc, "contents") else sc
        c1 = None if center1 is None else np.ascontiguousarray(center1, np.float64)
        nr = None if normals is None else np.ascontiguousarray(normals, np.float64)
        assert nr is None or nr.shape == (len(quads), 9)
        return s, (C.byref(s), None if c1 is None else c1.ctypes.data, C.addressof(quads), len(quads), None if nr is None else nr.ctypes.data), (c1, nr)

    def render(self, sc, quads, normals=None, center1=None, flat_bvh=False):
        """-> status (0; 1: the world was refused; 2: a normal was refused), rgb8, linear, segments, info = {DevScene::n_tris, entries with
        normals, the lowest refused entry}"""
        s, a, _keep = self._args(sc, center1, quads, normals)
        rgb, lin = np.zeros((s.height, s.width, 3), np.uint8), np.zeros((s.height, s.width, 3), np.float32)
        segs, info = C.c_uint64(), np.zeros(3, np.uint32)
        rc = self.L.lane_smooth_render(*a, int(flat_bvh), rgb.ctypes.data, lin.ctypes.data, C.addressof(segs), info.ctypes.data)
        return rc, rgb, lin, segs.value, [int(x) for x in info]

    def aovs(self, sc, quads, n, normals=None, center1=None, flat_bvh=False):
        s, a, _keep = self._args(sc, center1, quads, normals)
        out = np.zeros((s.height, s.width, 8), np.float32)
        return self.L.lane_smooth_aovs(*a, int(flat_bvh), n, out.ctypes.data), out


def load(abi):
    global _loaded
    if _loaded is None:
        d = tempfile.mkdtemp(prefix="lane_smooth_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "liblane_smooth.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS", "-shared",
                        os.path.join(ROOT, "tests", "smoothsim", "lane_smooth.cpp"), "-o", so], check=True)
        _loaded = LaneSmooth(C.CDLL(so), abi)
    return _loaded
