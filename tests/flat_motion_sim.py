"""The host build of flat primitives that move within the frame, tests/flatmotion/flat_motion_sim.cpp: load(abi) compiles it
once per session (g++, -ffp-contract=off, the walk's counters compiled in) and returns numpy wrappers.  TEST INFRASTRUCTURE."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from flat_bvh_sim import NODE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "flatmotion", "flat_motion_sim.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS"]
FLAT_BVH_BIT, FLAT_NORMALS_BIT, FLAT_MOTION_BIT = 0x80000000, 0x40000000, 0x20000000
COUNTS = ("rays_bvh", "rays_scan", "box_tests", "entry_tests", "nan_axes")
_loaded = None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data


class FlatMotionSim:
    def __init__(self, L, abi):
        self.L, self.abi = L, abi
        P, u32, u64, i32, f64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
        S = C.POINTER(abi.RtScene)
        L.fm_prepare.argtypes = [P, P, u32, P, P]
        L.fm_prepare.restype = None
        L.fm_hit_v.argtypes = [P, f64, P, i32, P, P, P, u64, P, P, P, P, P]
        L.fm_boxes.argtypes = [P, u32, P, P, P, P]
        L.fm_build.argtypes = [P, u32, P, P, u64, P, P, P]
        L.fm_list_hit.argtypes = [P, u32, P, u32, i32, P, P, P, P, u64, P, P, P]
        L.fm_list_surface.argtypes = [P, u32, P, P, u32, i32, P, P, P, P, u64] + [P] * 7
        L.fm_render.argtypes = [S, P, P, u32, P, P, i32, P, P, P, P, P]
        L.fm_aovs.argtypes = [S, P, P, u32, P, P, i32, u32, P, P]

    def prepare(self, quv, move):
        """-> kind (RT_FLAT_MOTION_*, -1: the entry itself is refused), records (n x 4)"""
        quv, move = _f64(quv).reshape(-1, 9), _f64(move).reshape(-1, 3)
        kind, rec = np.zeros(len(quv), np.int32), np.zeros((len(quv), 4))
        self.L.fm_prepare(quv.ctypes.data, move.ctypes.data, len(quv), kind.ctypes.data, rec.ctypes.data)
        return kind, rec

    def hit(self, quv, lim, m, rays, tau, closest, with_table=True):
        """one entry against n rays, each with its tau and closest -> status, hit, t, P, normal, front"""
        quv, m, rays, tau, closest = _f64(quv).reshape(9), _f64(m).reshape(3), _f64(rays), _f64(tau), _f64(closest)
        n = len(rays)
        hit, t, P, nrm, front = np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
        st = self.L.fm_hit_v(quv.ctypes.data, lim, m.ctypes.data, int(with_table), rays.ctypes.data, tau.ctypes.data, closest.ctypes.data, n,
                             hit.ctypes.data, t.ctypes.data, P.ctypes.data, nrm.ctypes.data, front.ctypes.data)
        return st, hit, t, P, nrm, front

    def boxes(self, flats, move):
        """flat_entry_box_swept of every entry -> ok (bool), lo, hi (n x 3; NaN rows where not ok)"""
        n, move = len(flats), _f64(move)
        ok, lo, hi = np.zeros(n, np.int32), np.full((n, 3), np.nan), np.full((n, 3), np.nan)
        assert self.L.fm_boxes(flats, n, move.ctypes.data, ok.ctypes.data, lo.ctypes.data, hi.ctypes.data) == 0
        lo[ok == 0], hi[ok == 0] = np.nan, np.nan
        return ok == 1, lo, hi

    def build(self, flats, move):
        """the host build of a moving list -> nodes (NODE records), order, always-visited entries, the motion table (n x 4; None: none moves)"""
        n, move = len(flats), _f64(move)
        info = np.zeros(3, np.uint32)
        assert self.L.fm_build(flats, n, move.ctypes.data, None, 0, None, None, info.ctypes.data) == 0
        nodes, order, motion = np.zeros(int(info[0]), NODE), np.zeros(n, np.uint32), np.zeros((n, 4))
        assert self.L.fm_build(flats, n, move.ctypes.data, nodes.ctypes.data, len(nodes), order.ctypes.data, motion.ctypes.data, info.ctypes.data) == 0
        return nodes, order, int(info[1]), (motion if info[2] else None)

    def list_hit(self, flats, move, rays, tau, closest, bvh, id_base=0, best_in=None):
        """flats_walk<true> over the whole list -> best, t, counts"""
        move, rays, closest = _f64(move), _f64(rays), _f64(closest)
        tau = np.ascontiguousarray(tau, np.float32)
        best_in = None if best_in is None else np.ascontiguousarray(best_in, np.int32)
        n = len(rays)
        best, t, count = np.zeros(n, np.int32), np.zeros(n), np.zeros(5, np.uint64)
        rc = self.L.fm_list_hit(flats, len(flats), move.ctypes.data, id_base, int(bvh), rays.ctypes.data, tau.ctypes.data, closest.ctypes.data, _ptr(best_in), n,
                                best.ctypes.data, t.ctypes.data, count.ctypes.data)
        assert rc == 0
        return best, t, dict(zip(COUNTS, (int(c) for c in count)))

    def list_surface(self, flats, move, rays, tau, closest, bvh, id_base=0, best_in=None, normals=None, out=None):
        """what rt_hip_flat_shutter_probe runs, in the host build: flats_hit through motion_tables at the ray's tau (f32), then
        object_surface<true> of a newly accepted flat entry -> {best, t, P, normal, front, origin} and the counts.  best is always written;
        the other outputs keep what `out` (a dict of arrays to write into) held wherever no such hit was accepted — zeros without `out`."""
        move, rays, closest, normals = _f64(move), _f64(rays), _f64(closest), _f64(normals)
        tau = None if tau is None else np.ascontiguousarray(tau, np.float32)
        best_in = None if best_in is None else np.ascontiguousarray(best_in, np.int32)
        n = len(rays)
        o = out if out is not None else dict(best=np.zeros(n, np.int32), t=np.zeros(n), P=np.zeros((n, 3)), normal=np.zeros((n, 3)),
                                             front=np.zeros(n, np.int32), origin=np.zeros((n, 3)))
        assert all(o[k].flags.c_contiguous and len(o[k]) == n for k in o)
        assert o["best"].dtype == o["front"].dtype == np.int32 and all(o[k].dtype == np.float64 for k in ("t", "P", "normal", "origin"))
        count = np.zeros(5, np.uint64)
        rc = self.L.fm_list_surface(flats, len(flats), _ptr(move), _ptr(normals), id_base, int(bvh), rays.ctypes.data, _ptr(tau), closest.ctypes.data,
                                    _ptr(best_in), n, o["best"].ctypes.data, o["t"].ctypes.data, o["P"].ctypes.data, o["normal"].ctypes.data,
                                    o["front"].ctypes.data, o["origin"].ctypes.data, count.ctypes.data)
        assert rc == 0, rc
        return o, dict(zip(COUNTS, (int(c) for c in count)))

    def _world(self, sc, center1, quads, normals, move):
        s = sc.contents if hasattr(sc, "contents") else sc
        c1, nr, mv = _f64(center1), _f64(normals), _f64(move)
        return s, (C.byref(s), _ptr(c1), C.addressof(quads), len(quads), _ptr(nr), _ptr(mv)), (c1, nr, mv)

    def render(self, sc, quads, move=None, normals=None, center1=None, flat_bvh=False):
        """the lane code's frame -> status, rgb8, linear, segments, info = {DevScene::n_tris, entries that move, lowest refused}, counts"""
        s, a, _keep = self._world(sc, center1, quads, normals, move)
        rgb, lin = np.zeros((s.height, s.width, 3), np.uint8), np.zeros((s.height, s.width, 3), np.float32)
        segs, info, count = C.c_uint64(), np.zeros(3, np.uint32), np.zeros(5, np.uint64)
        rc = self.L.fm_render(*a, int(flat_bvh), rgb.ctypes.data, lin.ctypes.data, C.addressof(segs), info.ctypes.data, count.ctypes.data)
        return rc, rgb, lin, segs.value, [int(x) for x in info], dict(zip(COUNTS, (int(c) for c in count)))

    def aovs(self, sc, quads, n, move=None, normals=None, center1=None, flat_bvh=False):
        """-> status, the first-hit records (h x w x 8 f32), the surface records (h x w: id u32, kind u32, t f64)"""
        s, a, _keep = self._world(sc, center1, quads, normals, move)
        out = np.zeros((s.height, s.width, 8), np.float32)
        surf = np.zeros((s.height, s.width), np.dtype([("id", "<u4"), ("kind", "<u4"), ("t", "<f8")]))
        return self.L.fm_aovs(*a, int(flat_bvh), n, out.ctypes.data, surf.ctypes.data), out, surf


def build_lib(flags=FLAGS, out_dir=None):
    d = out_dir or tempfile.mkdtemp(prefix="flat_motion_sim_")
    if out_dir is None:
        atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libflat_motion_sim.so")
    subprocess.run(["g++", *flags, "-shared", SRC, "-o", so], check=True)
    return so


def load(abi):
    global _loaded
    if _loaded is None:
        _loaded = FlatMotionSim(C.CDLL(build_lib()), abi)
    return _loaded
