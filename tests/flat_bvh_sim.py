"""The host build of the structure over the flat primitives, tests/flatbvh/flat_bvh_sim.cpp: load(abi) compiles it once per
session (g++, -ffp-contract=off, the walk's counters compiled in) and returns numpy wrappers.  `flats` is a ctypes array of abi.RtQuad
(flats_array makes one from quv rows and shapes)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = np.dtype([("lo", "<f8", 3), ("hi", "<f8", 3), ("skip", "<u4"), ("first", "<u4"), ("count", "<u4"), ("pad", "<u4")])   # rt_core.h FlatNode
assert NODE.itemsize == 64
# the preconditions of a ray (rt_core.h flat_ray_ok)
RAY_O_MAX, RAY_D_MAX = 2.0 ** 40, 2.0 ** 100
_loaded = None


def flats_array(abi, quvs, shapes=None, kind=0):
    """quv rows (n x 9) and shapes (None: all parallelograms; a scalar; or n values) as a ctypes array of abi.RtQuad"""
    quvs = np.ascontiguousarray(quvs, np.float64).reshape(-1, 9)
    n = len(quvs)
    shapes = np.zeros(n, np.uint32) if shapes is None else np.broadcast_to(np.asarray(shapes, np.uint32), (n,))
    out = (abi.RtQuad * n)()
    rec = np.frombuffer(out, np.uint8).reshape(n, C.sizeof(abi.RtQuad))
    rec[:, :72] = quvs.view(np.uint8).reshape(n, 72)
    for k in range(n):
        out[k].albedo[:] = [0.7, 0.6, 0.5]
        out[k].kind, out[k].fuzz_or_ior, out[k].reserved = kind, 1.5, int(shapes[k])
    return out


def ray_ok(rays):
    """flat_ray_ok restated: the rays (n x 6) the structure takes; every other takes the full scan"""
    with np.errstate(all="ignore"):
        o, d = np.abs(rays[:, :3]), np.abs(rays[:, 3:])
        return (o <= RAY_O_MAX).all(axis=1) & (d <= RAY_D_MAX).all(axis=1)


class FlatBvhSim:
    def __init__(self, L, abi):
        self.L, self.abi = L, abi
        P, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        S = C.POINTER(abi.RtScene)
        L.fb_build.argtypes = [P, u32, P, u64, P, P, C.c_char_p, u64]
        L.fb_entry_boxes.argtypes = [P, u32, P, P, P]
        L.fb_check.argtypes = [P, u64, P, u64, u32, C.c_char_p, u64]
        L.fb_hit_v.argtypes = [P, u32, u32, i32, P, P, P, u64, P, P, P]
        L.fb_surface_v.argtypes = [P, u32, u32, P, P, P, u64, P, P, P]
        L.fb_tie_v.argtypes = [P, C.c_double, P, P, P, u64] + [P] * 6
        L.fb_render.argtypes = [S, P, P, u32, i32, P, P, P, P]
        L.fb_scene_tables.argtypes = [S, P, P, u32, P, u64, P, P]

    def build(self, flats):
        """-> nodes (NODE records), order (u32), the number of always-visited entries; raises ValueError with the builder's message"""
        n = len(flats)
        info, msg = np.zeros(3, np.uint32), C.create_string_buffer(256)
        if self.L.fb_build(flats, n, None, 0, None, info.ctypes.data, msg, 256):
            raise ValueError(msg.value.decode())
        nodes, order = np.zeros(int(info[0]), NODE), np.zeros(n, np.uint32)
        assert self.L.fb_build(flats, n, nodes.ctypes.data, len(nodes), order.ctypes.data, info.ctypes.data, msg, 256) == 0
        return nodes, order, int(info[1])

    def entry_boxes(self, flats):
        """-> ok (bool per entry: inside the preconditions), lo, hi (n x 3, the padded boxes; NaN rows where not ok)"""
        n = len(flats)
        ok, lo, hi = np.zeros(n, np.int32), np.full((n, 3), np.nan), np.full((n, 3), np.nan)
        assert self.L.fb_entry_boxes(flats, n, ok.ctypes.data, lo.ctypes.data, hi.ctypes.data) == 0
        lo[ok == 0], hi[ok == 0] = np.nan, np.nan
        return ok == 1, lo, hi

    def check(self, nodes, order, n):
        """check_flat_bvh -> "" or the refusal"""
        nodes, order = np.ascontiguousarray(nodes, NODE), np.ascontiguousarray(order, np.uint32)
        msg = C.create_string_buffer(256)
        rc = self.L.fb_check(nodes.ctypes.data, len(nodes), order.ctypes.data, len(order), n, msg, 256)
        assert (rc == 0) == (msg.value == b"")
        return msg.value.decode()

    def hit(self, flats, rays, closest, bvh, id_base=0, best_in=None):
        """quads_hit over the whole list -> best, t (as returned), count = {rays_bvh, rays_scan, box_tests, entry_tests, nan_axes}"""
        rays, closest = np.ascontiguousarray(rays, np.float64), np.ascontiguousarray(closest, np.float64)
        n = len(rays)
        best_in = None if best_in is None else np.ascontiguousarray(best_in, np.int32)
        best, t, count = np.zeros(n, np.int32), np.zeros(n), np.zeros(5, np.uint64)
        rc = self.L.fb_hit_v(flats, len(flats), id_base, int(bvh), rays.ctypes.data, closest.ctypes.data, None if best_in is None else best_in.ctypes.data, n,
                             best.ctypes.data, t.ctypes.data, count.ctypes.data)
        assert rc == 0
        return best, t, dict(zip(("rays_bvh", "rays_scan", "box_tests", "entry_tests", "nan_axes"), (int(c) for c in count)))

    def surface(self, flats, rays, best, t, id_base=0):
        """the record of the accepted hits -> point (n x 3), normal (n x 3), front (zero rows where best < id_base)"""
        rays, best, t = np.ascontiguousarray(rays, np.float64), np.ascontiguousarray(best, np.int32), np.ascontiguousarray(t, np.float64)
        n = len(rays)
        point, normal, front = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
        assert self.L.fb_surface_v(flats, len(flats), id_base, rays.ctypes.data, best.ctypes.data, t.ctypes.data, n, point.ctypes.data, normal.ctypes.data,
                                   front.ctypes.data) == 0
        return point, normal, front

    def tie(self, quv, lim, rays, closest, tie_ok):
        """rt_flat_hit and rt_flat_hit_tie of one entry -> status, (hit, t, P) of each"""
        quv, rays, closest = np.ascontiguousarray(quv, np.float64).reshape(9), np.ascontiguousarray(rays, np.float64), np.ascontiguousarray(closest, np.float64)
        tie_ok = np.ascontiguousarray(np.broadcast_to(np.asarray(tie_ok, np.int32), (len(rays),)))
        n = len(rays)
        a = (np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 3)))
        b = (np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 3)))
        st = self.L.fb_tie_v(quv.ctypes.data, lim, rays.ctypes.data, closest.ctypes.data, tie_ok.ctypes.data, n, *(x.ctypes.data for x in a), *(x.ctypes.data for x in b))
        return st, a, b

    def render(self, sc, bvh, center1=None, quads=None):
        """the lane code's frame with (bvh) or without the structure -> status, rgb8, linear, segments, count"""
        s = sc.contents if hasattr(sc, "contents") else sc
        c1 = None if center1 is None else np.ascontiguousarray(center1, np.float64)
        rgb, lin = np.zeros((s.height, s.width, 3), np.uint8), np.zeros((s.height, s.width, 3), np.float32)
        segs, count = C.c_uint64(), np.zeros(5, np.uint64)
        rc = self.L.fb_render(C.byref(s), None if c1 is None else c1.ctypes.data, quads, 0 if quads is None else len(quads), int(bvh), rgb.ctypes.data,
                              lin.ctypes.data, C.addressof(segs), count.ctypes.data)
        return rc, rgb, lin, segs.value, dict(zip(("rays_bvh", "rays_scan", "box_tests", "entry_tests", "nan_axes"), (int(c) for c in count)))

    def scene_tables(self, sc, quads, center1=None):
        """the structure's tables of a world as a device scene must hold them -> nodes bytes, order bytes"""
        s = sc.contents if hasattr(sc, "contents") else sc
        c1 = None if center1 is None else np.ascontiguousarray(center1, np.float64)
        info = np.zeros(3, np.uint32)
        args = (C.byref(s), None if c1 is None else c1.ctypes.data, quads, len(quads))
        assert self.L.fb_scene_tables(*args, None, 0, None, info.ctypes.data) == 0
        nodes, order = np.zeros(int(info[0]), NODE), np.zeros(len(quads), np.uint32)
        assert self.L.fb_scene_tables(*args, nodes.ctypes.data, len(nodes), order.ctypes.data, info.ctypes.data) == 0
        return nodes.tobytes(), order.tobytes()


def load(abi):
    global _loaded
    if _loaded is None:
        d = tempfile.mkdtemp(prefix="flat_bvh_sim_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libflat_bvh_sim.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS", "-shared",
                        os.path.join(ROOT, "tests", "flatbvh", "flat_bvh_sim.cpp"), "-o", so], check=True)
        _loaded = FlatBvhSim(C.CDLL(so), abi)
    return _loaded
