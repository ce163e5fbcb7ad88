"""tests/trisim/ (csrc/common/rt_quad.h's rt_flat_hit and rt_tables.h's limit table, a g++ build with -ffp-contract=off): load() builds
tests/trisim/tri_sim.cpp once per session and returns numpy wrappers around its entry points."""
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


class TriSim:
    def __init__(self, L):
        self.L = L
        P, u64 = C.c_void_p, C.c_uint64
        L.flat_hit_v.argtypes = [P, C.c_double, P, P, u64] + [P] * 5
        L.quad_hit_v.argtypes = [P, P, P, u64] + [P] * 3
        L.tri_tables.argtypes = [P, P, C.c_uint32, P, u64, P, C.c_char_p, u64]

    def flat_hit_v(self, quv, lim, rays, closest):
        """rt_flat_hit / rt_quad_normal of rays (n x 6) against one flat primitive of limit lim -> rt_quad_prepare's status, hit, t, P, normal, front"""
        quv, rays, closest = _arr(quv).reshape(9), _arr(rays), _arr(closest)
        n = len(rays)
        hit, front = np.zeros(n, np.int32), np.zeros(n, np.int32)
        t, P, nrm = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        st = self.L.flat_hit_v(quv.ctypes.data, lim, rays.ctypes.data, closest.ctypes.data, n, hit.ctypes.data, t.ctypes.data, P.ctypes.data, nrm.ctypes.data,
                               front.ctypes.data)
        return st, hit, t, P, nrm, front

    def quad_hit_v(self, quv, rays, closest):
        """rt_quad_hit of the same build -> status, hit, t, P"""
        quv, rays, closest = _arr(quv).reshape(9), _arr(rays), _arr(closest)
        n = len(rays)
        hit, t, P = np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 3))
        st = self.L.quad_hit_v(quv.ctypes.data, rays.ctypes.data, closest.ctypes.data, n, hit.ctypes.data, t.ctypes.data, P.ctypes.data)
        return st, hit, t, P

    def tables(self, sc, quads):
        """build_tables through the C structs -> (the limit table, info = {len(quad_lim), n_tris, records, DevScene lim bound, DevScene n_tris}), or
        (None, build_tables' message) when it refused the world"""
        n = len(quads) if quads is not None else 0
        arr = (type(quads[0]) * n)(*quads) if n else None
        lim, info, msg = np.zeros(max(n, 1)), np.zeros(5, np.uint32), C.create_string_buffer(256)
        if self.L.tri_tables(C.addressof(sc), arr, n, lim.ctypes.data, n, info.ctypes.data, msg, 256):
            return None, msg.value.decode()
        return lim[:int(info[0])], info


def load():
    global _loaded
    if _loaded is None:
        d = tempfile.mkdtemp(prefix="tri_sim_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libtri_sim.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS", "-shared",
                        os.path.join(ROOT, "tests", "trisim", "tri_sim.cpp"), "-o", so], check=True)
        _loaded = TriSim(C.CDLL(so))
    return _loaded
