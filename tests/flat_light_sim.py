"""The host build of flat primitives that emit, tests/flatlight/flat_light_sim.cpp: load(abi) compiles it once per session
(g++, -ffp-contract=off) and returns numpy wrappers.  TEST INFRASTRUCTURE."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "flatlight", "flat_light_sim.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS"]
FLAT_BVH_BIT, FLAT_NORMALS_BIT, FLAT_MOTION_BIT, FLAT_LIGHTS_BIT = 0x80000000, 0x40000000, 0x20000000, 0x10000000
_loaded = None


def _arr(a, dt):
    return None if a is None else np.ascontiguousarray(a, dt)


def _ptr(a):
    return None if a is None else a.ctypes.data


class FlatLightSim:
    def __init__(self, L, abi):
        self.L, self.abi = L, abi
        P, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        S = C.POINTER(abi.RtScene)
        L.fl_aim.argtypes = [P, P, P, u64, P]
        L.fl_aim.restype = None
        L.fl_ab.argtypes = [P, u64, P]
        L.fl_ab.restype = None
        L.fl_words.argtypes = [P, u64, u64, P]
        L.fl_words.restype = None
        L.fl_emit_check.argtypes = [P, u32, P]
        L.fl_emit_check.restype = u32
        L.fl_render.argtypes = [S, P, P, u32, P, P, i32, P, P, P, P]
        L.fl_render_lens.argtypes = [S, P, P, u32, P, P, i32, P, P, P, P, P]
        L.fl_tables.argtypes = [S, P, u32, P, P, P, P, P, P]
        L.fl_aovs.argtypes = [S, P, P, u32, P, P, i32, u32, P, P]

    def aim(self, quv, triangle, words):
        """rt_flat_light_aim of n activations -> T (n x 3)"""
        quv, tri, words = _arr(quv, np.float64).reshape(-1, 9), _arr(triangle, np.int32), _arr(words, np.uint32).reshape(-1, 4)
        assert len(quv) == len(tri) == len(words)
        T = np.zeros((len(quv), 3))
        self.L.fl_aim(quv.ctypes.data, tri.ctypes.data, words.ctypes.data, len(quv), T.ctypes.data)
        return T

    def ab(self, words):
        """the (a, b) of the words before the fold -> n x 2"""
        words = _arr(words, np.uint32).reshape(-1, 4)
        out = np.zeros((len(words), 2))
        self.L.fl_ab(words.ctypes.data, len(words), out.ctypes.data)
        return out

    def words(self, act, seed):
        """the aim draw of n activations {pixel, sample, node of the hit, light j} -> n x 4 u32"""
        act = _arr(act, np.uint32).reshape(-1, 4)
        out = np.zeros((len(act), 4), np.uint32)
        self.L.fl_words(act.ctypes.data, len(act), int(seed), out.ctypes.data)
        return out

    def emit_check(self, emit):
        emit = _arr(emit, np.float32).reshape(-1, 3)
        n = C.c_uint32(0)
        bad = self.L.fl_emit_check(emit.ctypes.data, len(emit), C.byref(n))
        return int(bad), int(n.value)

    def _world(self, sc, center1, quads, normals, emit):
        s = sc.contents if hasattr(sc, "contents") else sc
        c1, nr, em = _arr(center1, np.float64), _arr(normals, np.float64), _arr(emit, np.float32)
        return s, (C.byref(s), _ptr(c1), C.addressof(quads), len(quads), _ptr(nr), _ptr(em)), (c1, nr, em)

    def render(self, sc, quads, emit=None, normals=None, center1=None, flat_bvh=False, lens=None):
        """the lane code's frame -> status, rgb8, linear, segments, info = {DevScene::n_tris, emitters, n_lights}"""
        s, a, _keep = self._world(sc, center1, quads, normals, emit)
        rgb, lin = np.zeros((s.height, s.width, 3), np.uint8), np.zeros((s.height, s.width, 3), np.float32)
        segs, info = C.c_uint64(), np.zeros(3, np.uint32)
        if lens is not None:   # (u, v, radius) as tests/test_medium_gpu._load returns it
            lz = np.ascontiguousarray(list(lens[0]) + list(lens[1]) + [lens[2]], np.float64)
            rc = self.L.fl_render_lens(*a, int(flat_bvh), lz.ctypes.data, rgb.ctypes.data, lin.ctypes.data, C.addressof(segs), info.ctypes.data)
        else:
            rc = self.L.fl_render(*a, int(flat_bvh), rgb.ctypes.data, lin.ctypes.data, C.addressof(segs), info.ctypes.data)
        return rc, rgb, lin, segs.value, [int(x) for x in info]

    def tables(self, sc, quads, emit=None):
        """the world's material records and light list as the kernels read them -> status, {"mat", "matc", "lights"} (bytes), info"""
        s = sc.contents if hasattr(sc, "contents") else sc
        em = _arr(emit, np.float32)
        sizes, info = np.zeros(3, np.uint64), np.zeros(3, np.uint32)
        rc = self.L.fl_tables(C.byref(s), C.addressof(quads), len(quads), _ptr(em), None, None, None, sizes.ctypes.data, info.ctypes.data)
        if rc:
            return rc, None, [int(x) for x in info]
        mat, matc, lights = np.zeros(int(sizes[0]), np.uint8), np.zeros(int(sizes[1]), np.uint8), np.zeros(max(1, int(sizes[2])), np.uint32)
        rc = self.L.fl_tables(C.byref(s), C.addressof(quads), len(quads), _ptr(em), mat.ctypes.data, matc.ctypes.data, lights.ctypes.data, sizes.ctypes.data,
                              info.ctypes.data)
        return rc, {"mat": mat.tobytes(), "matc": matc.tobytes(), "lights": lights[:int(sizes[2])].tobytes()}, [int(x) for x in info]

    def aovs(self, sc, quads, n, emit=None, normals=None, center1=None, flat_bvh=False):
        """-> status, the first-hit records (h x w x 8 f32), the surface records (h x w: id u32, kind u32, t f64)"""
        s, a, _keep = self._world(sc, center1, quads, normals, emit)
        out = np.zeros((s.height, s.width, 8), np.float32)
        surf = np.zeros((s.height, s.width), np.dtype([("id", "<u4"), ("kind", "<u4"), ("t", "<f8")]))
        return self.L.fl_aovs(*a, int(flat_bvh), n, out.ctypes.data, surf.ctypes.data), out, surf


def build_lib(flags=FLAGS, out_dir=None):
    d = out_dir or tempfile.mkdtemp(prefix="flat_light_sim_")
    if out_dir is None:
        atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libflat_light_sim.so")
    subprocess.run(["g++", *flags, "-shared", SRC, "-o", so], check=True)
    return so


def load(abi):
    global _loaded
    if _loaded is None:
        _loaded = FlatLightSim(C.CDLL(build_lib()), abi)
    return _loaded
