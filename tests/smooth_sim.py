"""tests/smoothsim/ (csrc/common/rt_flat_normal.h, a g++ build with -ffp-contract=off): load() builds tests/smoothsim/smooth_sim.cpp once per
session and returns numpy wrappers around its entry points."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_loaded = None


def _arr(a):
    return np.ascontiguousarray(a, np.float64)


class SmoothSim:
    def __init__(self, L):
        self.L = L
        P, u64 = C.c_void_p, C.c_uint64
        L.smooth_prepare_v.argtypes = [P, u64, P, P]
        L.smooth_shade_v.argtypes = [P, P, P, P, u64, P, P]
        L.smooth_shade_each.argtypes = [P, P, P, P, u64, P, P, P]
        L.smooth_unit_1d.argtypes = [C.c_double]
        L.smooth_unit_1d.restype = C.c_double

    def prepare(self, normals):
        """rt_flat_normal_prepare of [n, 9] -> kind [n] (0 flat, 1 smooth, 2 refused), records [n, 9]"""
        a = _arr(normals).reshape(-1, 9)
        kind, rec = np.zeros(len(a), np.int32), np.zeros((len(a), 9))
        self.L.smooth_prepare_v(a.ctypes.data, len(a), kind.ctypes.data, rec.ctypes.data)
        return kind, rec

    def shade(self, quv, rec, d, P):
        """rt_flat_normal_shade of n hits (d, P: [n, 3]) on one entry -> rt_quad_prepare's status, normal [n, 3], fell [n]"""
        quv, rec, d, P = _arr(quv).reshape(9), _arr(rec).reshape(9), _arr(d), _arr(P)
        n = len(d)
        nrm, fell = np.zeros((n, 3)), np.zeros(n, np.int32)
        st = self.L.smooth_shade_v(quv.ctypes.data, rec.ctypes.data, d.ctypes.data, P.ctypes.data, n, nrm.ctypes.data, fell.ctypes.data)
        return st, nrm, fell

    def shade_each(self, quv, rec, d, P):
        """the same with one entry per hit (quv, rec: [n, 9]) -> normal, fell (-1: the entry was refused), status"""
        quv, rec, d, P = _arr(quv).reshape(-1, 9), _arr(rec).reshape(-1, 9), _arr(d), _arr(P)
        n = len(d)
        nrm, fell, st = np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.L.smooth_shade_each(quv.ctypes.data, rec.ctypes.data, d.ctypes.data, P.ctypes.data, n, nrm.ctypes.data, fell.ctypes.data, st.ctypes.data)
        return nrm, fell, st

    def unit_1d(self, y):
        return self.L.smooth_unit_1d(float(y))


def load():
    global _loaded
    if _loaded is None:
        d = tempfile.mkdtemp(prefix="smooth_sim_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libsmooth_sim.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                        os.path.join(ROOT, "tests", "smoothsim", "smooth_sim.cpp"), "-o", so], check=True)
        _loaded = SmoothSim(C.CDLL(so))
    return _loaded
