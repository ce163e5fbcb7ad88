"""The CPU lane simulator of tests/lanesim/ (rt_core.h's per-lane code and rt_tables.h, a g++ build with -ffp-contract=off): load(abi) builds
tests/lanesim/lane_sim.cpp once per session and returns numpy wrappers around its entry points.  A scene argument is an RtScene or a
pointer to one; center1 (n_spheres x 3, or None), quads (a ctypes array of RtQuad, or None) and every other array may be None where the
C side takes a null pointer.  Calls that can be refused return their status first: the tests assert it."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURF = np.dtype([("id", "<u4"), ("kind", "<u4"), ("t", "<f8")])   # rt_core.h SurfRec
_loaded = None


def _ptr(a):
    return None if a is None else a.ctypes.data


def _arr(a, dtype=np.float64):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _scene(sc):
    return sc.contents if hasattr(sc, "contents") else sc


class LaneSim:
    F_MEDIUM, F_SOLID, F_QUADS = 1, 2, 4        # lane_sim.h: the bits of features_or

    def __init__(self, L, abi):
        self.L = L
        S, Q, P, u32, u64 = C.POINTER(abi.RtScene), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64
        world = [S, P, Q, u32]                        # scene, center1, quads, n_quads
        L.lane_sim_render.argtypes = world + [u32, P, P, P]
        L.lane_sim_aovs.argtypes = world + [u32, u32, P]
        L.lane_sim_surface.argtypes = world + [P]
        L.lane_sim_hit_world_v.argtypes = world + [P, P, P, u64, P, P, P]
        L.lane_sim_tables.argtypes = world + [P, P, u64]
        L.lane_sim_tables.restype = C.c_int64
        L.lane_sim_tables_error.argtypes = world + [C.c_char_p, u64]
        L.motion_table.argtypes = [S, P, P, P]
        L.medium_tables.argtypes = [S, P, P, P, P]
        L.medium_cell_lists.argtypes = [S, P, u32]
        L.medium_neg_log_v.argtypes = [P, u64, P]
        L.medium_terms_v.argtypes = [P, P, P, P, u64, u64, P]
        L.solid_checker_v.argtypes = [P, u64, P]
        L.solid_noise_v.argtypes = [P, u64, u32, P]
        L.solid_factor_v.argtypes = [P, u64, u32, u32, u32, P]
        L.solid_albedo_v.argtypes = [S, u32, P, u64, P]
        L.quad_prepare_v.argtypes = [P, u64, P, P]
        L.quad_hit_v.argtypes = [P, P, P, u64] + [P] * 5
        L.quad_box.argtypes = [P] * 3
        for f in (L.lane_sim_tables_error, L.medium_neg_log_v, L.medium_terms_v, L.solid_checker_v, L.solid_noise_v, L.solid_factor_v, L.quad_prepare_v, L.quad_box):
            f.restype = None

    @staticmethod
    def _world(sc, center1, quads, n_quads=None):
        """the four leading arguments of the lane_sim_* calls (and the arrays they point into, to keep them alive)"""
        c1 = _arr(center1)
        return (C.byref(_scene(sc)), _ptr(c1), quads, (len(quads) if quads is not None else 0) if n_quads is None else n_quads), c1

    # -------------------------------------------------------------- the lane code
    def render(self, sc, center1=None, quads=None, features_or=0):
        """-> status, rgb8, linear (height x width x 3), segments; the instantiation by the scene's content | features_or (lane_sim.h)"""
        s = _scene(sc)
        rgb, lin, segs = np.zeros((s.height, s.width, 3), np.uint8), np.zeros((s.height, s.width, 3), np.float32), C.c_uint64()
        w, _keep = self._world(sc, center1, quads)
        return self.L.lane_sim_render(*w, features_or, rgb.ctypes.data, lin.ctypes.data, C.addressof(segs)), rgb, lin, segs.value

    def aovs(self, sc, n, center1=None, quads=None, features_or=0):
        """-> status, the first-hit records of n samples per pixel (height x width x 8 f32)"""
        s = _scene(sc)
        out = np.zeros((s.height, s.width, 8), np.float32)
        w, _keep = self._world(sc, center1, quads)
        return self.L.lane_sim_aovs(*w, features_or, n, out.ctypes.data), out

    def surface(self, sc, center1=None, quads=None):
        """-> status, the surface record of every pixel (height x width, dtype SURF)"""
        s = _scene(sc)
        out = np.zeros((s.height, s.width), SURF)
        w, _keep = self._world(sc, center1, quads)
        return self.L.lane_sim_surface(*w, out.ctypes.data), out

    def hit_world_v(self, sc, rays, center1=None, quads=None, tau=None, node=None, miss_t=None):
        """hit_world of rays (n x 6) at shutter times tau (None: 0) -> status, best, t, work (n x 2 = exact tests, grid steps).  node
        (None: walk without the medium candidate) is each ray's RNG node.  A miss has best -1 and t as the walk left it (the largest
        double), or miss_t where one is given."""
        rays, tau, node = _arr(rays), _arr(tau, np.float32), _arr(node, np.uint32)
        best, t, work = np.zeros(len(rays), np.int32), np.zeros(len(rays)), np.zeros((len(rays), 2), np.uint32)
        w, _keep = self._world(sc, center1, quads)
        rc = self.L.lane_sim_hit_world_v(*w, rays.ctypes.data, _ptr(tau), _ptr(node), len(rays), best.ctypes.data, t.ctypes.data, work.ctypes.data)
        if miss_t is not None:
            t[best < 0] = miss_t
        return rc, best, t, work

    # -------------------------------------------------------------- the tables
    def tables_blob(self, sc, center1=None, quads=None, n_quads=None):
        """-> every table build_tables fills as one length-prefixed blob (bytes; None when build_tables refused the world),
        info = {n_solids, n_media, n_moving, wide, n_quads, simple_colour}"""
        w, _keep = self._world(sc, center1, quads, n_quads)
        info = np.zeros(6, np.uint32)
        size = self.L.lane_sim_tables(*w, info.ctypes.data, None, 0)
        if size < 0:
            return None, info
        buf = np.zeros(size, np.uint8)
        assert self.L.lane_sim_tables(*w, info.ctypes.data, buf.ctypes.data, size) == size
        return buf.tobytes(), info

    def tables(self, sc, center1=None, quads=None, n_quads=None):
        """-> the blob's parts (geom, mat, matc, cell_word, cell_items, cell_items32, large, large_geom, motion, medium, lights, quads, then
        the GridDesc and the counts; None when build_tables refused the world), info, build_tables' message"""
        blob, info = self.tables_blob(sc, center1, quads, n_quads)
        if blob is None:
            w, _keep = self._world(sc, center1, quads, n_quads)
            msg = C.create_string_buffer(256)
            self.L.lane_sim_tables_error(*w, msg, 256)
            return None, info, msg.value.decode()
        parts, at = [], 0
        for _ in range(12):
            n = int.from_bytes(blob[at:at + 8], "little")
            parts.append(blob[at + 8:at + 8 + n])
            at += 8 + n
        parts.append(blob[at:])
        return parts, info, ""

    def motion_table(self, sc, center1):
        """-> status (2: a static world, no table), the dv table (n x 4), info = {n_moving, grid n[0..2], n_large, n_items, wide}"""
        n = _scene(sc).n_spheres
        out, info, c1 = np.zeros((max(n, 1), 4), np.float64), np.zeros(8, np.uint32), _arr(center1)
        return self.L.motion_table(C.byref(_scene(sc)), _ptr(c1), out.ctypes.data, info.ctypes.data), out[:n], info

    def medium_tables(self, sc, center1=None):
        """-> status, info = {n_media, grid n[0..2], n_large, n_items, wide}, the number of cells that list each sphere, is it `large`"""
        n = _scene(sc).n_spheres
        info, listed, is_large, c1 = np.zeros(8, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), _arr(center1)
        return self.L.medium_tables(C.byref(_scene(sc)), _ptr(c1), info.ctypes.data, listed.ctypes.data, is_large.ctypes.data), info, listed, is_large

    def medium_cell_lists(self, sc, p, idx):
        return self.L.medium_cell_lists(C.byref(_scene(sc)), _arr(p).ctypes.data, idx)

    # -------------------------------------------------------------- rt_neg_log.h, rt_solid.h, rt_quad.h built for the host
    def _vec(self, fn, dtype, p, *args):
        p = _arr(p)
        out = np.zeros(len(p), dtype)
        fn(p.ctypes.data, len(p), *args, out.ctypes.data)
        return out

    def medium_neg_log_v(self, x):
        return self._vec(self.L.medium_neg_log_v, np.float64, x)

    def medium_terms_v(self, rays, spheres, density, addr, seed):
        """what medium_hit decides on for n (ray, sphere {centre, radius}, density, address {pixel, node, sphere index}) -> n x 8 {disc, t1,
        t2, inside, u, dist, fast, stage} (lane_sim.cpp medium_terms_v; stage 0: no disc, 1: no t_in < t2, 2: dist > inside, 3: a candidate)"""
        rays, spheres, density, addr = _arr(rays), _arr(spheres), _arr(density), _arr(addr, np.uint32)
        assert rays.shape == (len(rays), 6) and spheres.shape == (len(rays), 4) and density.shape == (len(rays),) and addr.shape == (len(rays), 3)
        out = np.zeros((len(rays), 8))
        self.L.medium_terms_v(rays.ctypes.data, spheres.ctypes.data, density.ctypes.data, addr.ctypes.data, seed, len(rays), out.ctypes.data)
        return out

    def solid_checker_v(self, p):
        return self._vec(self.L.solid_checker_v, np.int32, p)

    def solid_noise_v(self, p, seed):
        return self._vec(self.L.solid_noise_v, np.float64, p, seed)

    def solid_factor_v(self, p, mode, octaves, seed):
        return self._vec(self.L.solid_factor_v, np.float64, p, mode, octaves, seed)

    def solid_albedo_v(self, sc, idx, points):
        """-> status, solid_albedo (n x 3 f32) of world-space points on sphere idx"""
        points = _arr(points)
        colour = np.zeros((len(points), 3), np.float32)
        return self.L.solid_albedo_v(C.byref(_scene(sc)), idx, points.ctypes.data, len(points), colour.ctypes.data), colour

    def quad_prepare_v(self, quv):
        """rt_quad_prepare of quv (n x 9: q, u, v) -> the records (n x 16 doubles), its return values"""
        quv = _arr(quv)
        rec, st = np.zeros((len(quv), 16)), np.zeros(len(quv), np.int32)
        self.L.quad_prepare_v(quv.ctypes.data, len(quv), rec.ctypes.data, st.ctypes.data)
        return rec, st

    def quad_hit_v(self, quv, rays, closest):
        """rt_quad_hit / rt_quad_normal of rays (n x 6) against one quad -> rt_quad_prepare's status, hit, t, P, normal, front"""
        quv, rays, closest = _arr(quv).reshape(9), _arr(rays), _arr(closest)
        n = len(rays)
        hit, front = np.zeros(n, np.int32), np.zeros(n, np.int32)
        t, P, nrm = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        st = self.L.quad_hit_v(quv.ctypes.data, rays.ctypes.data, closest.ctypes.data, n, hit.ctypes.data, t.ctypes.data, P.ctypes.data, nrm.ctypes.data,
                               front.ctypes.data)
        return st, hit, t, P, nrm, front

    def quad_box(self, mn, mx):
        mn, mx, out = _arr(mn), _arr(mx), np.zeros((6, 9))
        self.L.quad_box(mn.ctypes.data, mx.ctypes.data, out.ctypes.data)
        return out


def load(abi):
    global _loaded
    if _loaded is None:
        d = tempfile.mkdtemp(prefix="lane_sim_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "liblane_sim.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS", "-shared",
                        os.path.join(ROOT, "tests", "lanesim", "lane_sim.cpp"), "-o", so], check=True)
        _loaded = LaneSim(C.CDLL(so), abi)
    return _loaded
