"""The host build of images on flat primitives, tests/flatimage/flat_image_sim.cpp: load(abi) compiles it once per session
(g++, -ffp-contract=off) and returns numpy wrappers.  TEST INFRASTRUCTURE."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "flatimage", "flat_image_sim.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS"]
FLAT_BVH_BIT, FLAT_NORMALS_BIT, FLAT_MOTION_BIT, FLAT_LIGHTS_BIT, FLAT_IMAGES_BIT = 0x80000000, 0x40000000, 0x20000000, 0x10000000, 0x08000000
REC = np.dtype([("texel_off", "<u4"), ("W", "<u4"), ("H", "<u4"), ("wrap", "<u4"), ("uv", "<f8", (6,))])    # the resident record, 64 B
_loaded = None


def _arr(a, dt):
    return None if a is None else np.ascontiguousarray(a, dt)


def _ptr(a):
    return None if a is None else a.ctypes.data


def records(W, H, wrap, uv, texel_off=0):
    """n resident records from per-hit columns"""
    n = len(uv)
    r = np.zeros(n, REC)
    r["texel_off"], r["W"], r["H"], r["wrap"], r["uv"] = texel_off, W, H, wrap, uv
    return r


class FlatImageSim:
    def __init__(self, L, abi):
        self.L, self.abi = L, abi
        P, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        S = C.POINTER(abi.RtScene)
        L.fi_texel.argtypes = [P, P, P, u64, P]
        L.fi_texel.restype = None
        L.fi_colour.argtypes = [P, u64, P]
        L.fi_colour.restype = None
        L.fi_albedo.argtypes = [P, P, P, P, P, u64, P]
        L.fi_albedo.restype = None
        L.fi_tex_table.argtypes = [S, P]
        L.fi_tex_table.restype = None
        L.fi_prepare.argtypes = [P, u32, P, u32, P, P, P]
        L.fi_prepare.restype = None
        L.fi_render.argtypes = [S, P, P, u32, P, P, P, P, i32, P, P, P, P, P]
        L.fi_aovs.argtypes = [S, P, P, u32, P, P, P, P, i32, u32, P]

    def texel(self, rec, ouvw, P):
        """rt_flat_image_texel of n hits -> n x 3 u32 {col, row, index}"""
        rec, ouvw, P = np.ascontiguousarray(rec), _arr(ouvw, np.float64).reshape(-1, 12), _arr(P, np.float64).reshape(-1, 3)
        assert rec.dtype == REC and len(rec) == len(ouvw) == len(P)
        out = np.zeros((len(rec), 3), np.uint32)
        self.L.fi_texel(rec.ctypes.data, ouvw.ctypes.data, P.ctypes.data, len(rec), out.ctypes.data)
        return out

    def colour(self, words):
        words = _arr(words, np.uint32)
        out = np.zeros((len(words), 3), np.float32)
        self.L.fi_colour(words.ctypes.data, len(words), out.ctypes.data)
        return out

    def albedo(self, rec, quv, tex4, origin, P):
        """flat_image_albedo on a one-entry table -> n x 3 f32"""
        rec, quv, tex4 = np.ascontiguousarray(rec), _arr(quv, np.float64), _arr(tex4, np.uint32)
        origin, P = _arr(origin, np.float64).reshape(-1, 3), _arr(P, np.float64).reshape(-1, 3)
        out = np.zeros((len(P), 3), np.float32)
        self.L.fi_albedo(rec.ctypes.data, quv.ctypes.data, tex4.ctypes.data, origin.ctypes.data, P.ctypes.data, len(P), out.ctypes.data)
        return out

    def tex_table(self, sc):
        s = sc.contents if hasattr(sc, "contents") else sc
        out = np.zeros((max(1, s.n_textures), 4), np.uint32)
        self.L.fi_tex_table(C.byref(s), out.ctypes.data)
        return out[:s.n_textures]

    def prepare(self, images, table, kind, fill=0):
        """the host path -> records (n, pre-filled), codes"""
        n = len(images)
        table, kind = _arr(table, np.uint32).reshape(-1, 4), _arr(kind, np.uint32)
        out = np.full((n, 8), fill, np.uint64)
        code = np.zeros(n, np.int32)
        self.L.fi_prepare(C.addressof(images), n, table.ctypes.data, len(table), kind.ctypes.data, out.ctypes.data, code.ctypes.data)
        return out, code

    def _world(self, w):
        sc = w["sc"].c
        c1, nr, mv, em = _arr(w["c1"], np.float64), _arr(w["normals"], np.float64), _arr(w["move"], np.float64), _arr(w["emit"], np.float32)
        im = w["images"]
        return sc, (C.byref(sc), _ptr(c1), C.addressof(w["quads"]), len(w["quads"]), _ptr(nr), _ptr(mv), _ptr(em), C.addressof(im) if im is not None else None), (c1, nr, mv, em)

    def render(self, w, flat_bvh=False):
        """the lane code's frame of a world of tests/flat_image_frames.py -> status, rgb8, linear, segments, info"""
        s, a, _keep = self._world(w)
        rgb, lin = np.zeros((s.height, s.width, 3), np.uint8), np.zeros((s.height, s.width, 3), np.float32)
        segs, info = C.c_uint64(), np.zeros(4, np.uint32)
        lz = None
        if w["lens"] is not None:
            lens = w["lens"]
            lz = np.ascontiguousarray(list(lens[0]) + list(lens[1]) + [lens[2]], np.float64)
        rc = self.L.fi_render(*a, int(flat_bvh), _ptr(lz), rgb.ctypes.data, lin.ctypes.data, C.addressof(segs), info.ctypes.data)
        return rc, rgb, lin, segs.value, [int(x) for x in info]

    def aovs(self, w, n, flat_bvh=False):
        s, a, _keep = self._world(w)
        out = np.zeros((s.height, s.width, 8), np.float32)
        return self.L.fi_aovs(*a, int(flat_bvh), n, out.ctypes.data), out


def build_lib(flags=FLAGS, out_dir=None):
    d = out_dir or tempfile.mkdtemp(prefix="flat_image_sim_")
    if out_dir is None:
        atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libflat_image_sim.so")
    subprocess.run(["g++", *flags, "-shared", SRC, "-o", so], check=True)
    return so


def load(abi):
    global _loaded
    if _loaded is None:
        _loaded = FlatImageSim(C.CDLL(build_lib()), abi)
    return _loaded
