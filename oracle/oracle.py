"""ctypes binding of oracle/librt_oracle.so — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_INDEP = None


class RtOracleExt(C.Structure):
    """rt_oracle.h's RtOracleExt: moving spheres and the thin lens"""
    _fields_ = [("center1", C.POINTER(C.c_double)), ("lens_u", C.POINTER(C.c_double)), ("lens_v", C.POINTER(C.c_double)), ("lens_r", C.c_double)]


def make_ext(scene_ptr, center1=None, lens=None):
    """-> (RtOracleExt or None, the arrays it points into): center1 = n_spheres x 3 centres at shutter close (anything numpy takes, or
    a pointer to doubles such as host.Scene.center1()'s), lens = (u, v, r) as rt_hip_set_lens takes them"""
    if center1 is None and lens is None:
        return None, ()
    ext, keep = RtOracleExt(), []
    if center1 is not None:
        n = scene_ptr.contents.n_spheres
        if isinstance(center1, C.POINTER(C.c_double)):
            center1 = np.ctypeslib.as_array(center1, shape=(n * 3,))
        c1 = np.ascontiguousarray(np.array(center1, dtype=np.float64).reshape(-1))
        assert c1.size == 3 * n, (c1.size, n)
        keep.append(c1)
        ext.center1 = c1.ctypes.data_as(C.POINTER(C.c_double))
    if lens is not None:
        u, v, r = lens
        lu, lv = (C.c_double * 3)(*u), (C.c_double * 3)(*v)
        keep += [lu, lv]
        ext.lens_u, ext.lens_v, ext.lens_r = lu, lv, float(r)
    return ext, keep


def build():
    subprocess.run(["make", "-C", _HERE, "-s"], check=True)


def lib(abi):
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "librt_oracle.so")
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.rt_oracle_render.argtypes = [C.POINTER(abi.RtScene), C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_void_p,
                                       C.POINTER(abi.RtStats), C.c_int]
        L.rt_oracle_render_window.argtypes = [C.POINTER(abi.RtScene), C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.POINTER(abi.RtStats), C.c_int]
        L.rt_oracle_accumulate.argtypes = [C.POINTER(abi.RtScene), C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.POINTER(abi.RtStats), C.c_int]
        L.rt_oracle_render_window_ext.argtypes = [C.POINTER(abi.RtScene), C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_uint32, C.POINTER(RtOracleExt),
                                                  C.c_void_p, C.c_void_p, C.POINTER(abi.RtStats), C.c_int]
        L.rt_oracle_accumulate_ext.argtypes = [C.POINTER(abi.RtScene), C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(RtOracleExt), C.c_void_p, C.POINTER(abi.RtStats), C.c_int]
        L.rt_oracle_camera_ray_ext.argtypes = [C.POINTER(abi.RtScene), C.POINTER(RtOracleExt), C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_double)]
        L.rt_oracle_render_rays.argtypes = [C.POINTER(abi.RtScene), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.RtStats), C.c_int]
        L.rt_oracle_philox4x32_10.argtypes = [C.POINTER(C.c_uint32)] * 3
        L.rt_oracle_philox4x32_10.restype = None
        L.rt_oracle_sphere_hit.argtypes = [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.rt_oracle_refract.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]
        L.rt_oracle_refract.restype = None
        L.rt_oracle_reflect.argtypes = [C.POINTER(C.c_double)] * 3
        L.rt_oracle_reflect.restype = None
        L.rt_oracle_reflectance.argtypes = [C.c_double, C.c_double]
        L.rt_oracle_reflectance.restype = C.c_double
        L.rt_oracle_camera_new.argtypes = [C.POINTER(C.c_double)] * 3 + [C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.rt_oracle_camera_new.restype = None
        L.rt_oracle_get_ray.argtypes = [C.POINTER(abi.RtScene), C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.rt_oracle_get_ray.restype = None
        L.rt_oracle_ray_color.argtypes = [C.POINTER(abi.RtScene), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.rt_oracle_ray_color.restype = None
        L.rt_oracle_texture_albedo.argtypes = [C.POINTER(abi.RtSphere), C.POINTER(abi.RtTexture), C.c_double, C.c_double, C.POINTER(C.c_float)]
        L.rt_oracle_texture_albedo.restype = None
        L.rt_oracle_f32_to_u8.argtypes = [C.c_float]
        L.rt_oracle_f32_to_u8.restype = C.c_uint8
        L.rt_oracle_find_lights.argtypes = [C.POINTER(abi.RtSphere), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
        L.rt_oracle_find_lights.restype = C.c_uint32
        L.rt_oracle_draws.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.rt_oracle_draws.restype = None
        L.rt_oracle_threads.restype = C.c_int
        L.rt_oracle_p3_op.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]
        L.rt_oracle_ray_at.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]
        L.rt_oracle_ray_at.restype = None
        L.rt_oracle_atan2_v.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.rt_oracle_atan2_v.restype = None
        L.rt_oracle_atan2.argtypes = [C.c_double, C.c_double]
        L.rt_oracle_atan2.restype = C.c_double
        _LIB = L
    return _LIB


def indep_lib(abi):
    """librt_oracle_indep.so: the restatement with the light-sampling draw on a Philox block of its own (round 3's addressing);
    an independent reference for STATISTICS of the shipped addressing (tests/test_light_draw_statistics.py), never for parity"""
    global _INDEP
    if _INDEP is None:
        path = os.path.join(_HERE, "librt_oracle_indep.so")
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.rt_oracle_render_window.argtypes = [C.POINTER(abi.RtScene), C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.POINTER(abi.RtStats), C.c_int]
        _INDEP = L
    return _INDEP


def render(abi, scene_ptr, tiles=None, n_threads=0, want_linear=True, x_range=None, independent_light_draw=False, center1=None, lens=None):
    """-> (rgb8 [rows,w,3] u8, linear [rows,w,3] f32 | None, stats dict); x_range = (x0, x1): only those pixels
    of the rows are rendered (the rest of the arrays stays 0).  center1 / lens (make_ext): the frame with moving spheres and / or
    through a thin lens, by rt_oracle_render_window_ext; without them the call is rt_oracle_render_window's, as ever."""
    sc = scene_ptr.contents
    rows = abi.tiles_local_rows(sc.height, tiles)
    rgb = np.zeros((rows, sc.width, 3), np.uint8)
    lin = np.zeros((rows, sc.width, 3), np.float32) if want_linear else None
    st = abi.RtStats()
    x0, x1 = x_range if x_range is not None else (0, sc.width)
    ext, _keep = make_ext(scene_ptr, center1, lens)
    if ext is not None:
        assert not independent_light_draw
        rc = lib(abi).rt_oracle_render_window_ext(scene_ptr, C.byref(tiles) if tiles is not None else None, x0, x1, C.byref(ext), rgb.ctypes.data,
                                                  lin.ctypes.data if lin is not None else None, C.byref(st), n_threads)
        if rc != 0:
            raise RuntimeError(f"rt_oracle_render_window_ext failed: {rc}")
        return rgb, lin, st.as_dict()
    rc = (indep_lib(abi) if independent_light_draw else lib(abi)).rt_oracle_render_window(scene_ptr, C.byref(tiles) if tiles is not None else None, x0, x1, rgb.ctypes.data,
                                          lin.ctypes.data if lin is not None else None, C.byref(st), n_threads)
    if rc != 0:
        raise RuntimeError(f"rt_oracle_render failed: {rc}")
    return rgb, lin, st.as_dict()


def render_rays(abi, scene_ptr, rays, n_threads=0):
    """render() of the whole frame with the camera ray of every sample of pixel (y, x) taken from rays[y, x] = (origin, direction)
    -> (rgb8 [h,w,3] u8, linear [h,w,3] f32, stats dict)"""
    sc = scene_ptr.contents
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    assert rays.shape == (sc.height, sc.width, 6), rays.shape
    rgb = np.zeros((sc.height, sc.width, 3), np.uint8)
    lin = np.zeros((sc.height, sc.width, 3), np.float32)
    st = abi.RtStats()
    rc = lib(abi).rt_oracle_render_rays(scene_ptr, rays.ctypes.data, rgb.ctypes.data, lin.ctypes.data, C.byref(st), n_threads)
    if rc != 0:
        raise RuntimeError(f"rt_oracle_render_rays failed: {rc}")
    return rgb, lin, st.as_dict()


def accumulate(abi, scene_ptr, begin, count, accum=None, tiles=None, x_range=None, n_threads=0, center1=None, lens=None):
    """samples [begin, begin + count) of every pixel ADDED into accum by include/rt_abi.h's accumulator rule (rows x width x 3
    uint64, packed like the RGB8 frame; None: a zeroed one) -> (accum, stats dict).  x_range = (x0, x1): only those pixels.
    center1 / lens: as render's (rt_oracle_accumulate_ext)."""
    sc = scene_ptr.contents
    rows = abi.tiles_local_rows(sc.height, tiles)
    if accum is None:
        accum = np.zeros((rows, sc.width, 3), np.uint64)
    assert accum.dtype == np.uint64 and accum.shape == (rows, sc.width, 3) and accum.flags.c_contiguous
    st = abi.RtStats()
    x0, x1 = x_range if x_range is not None else (0, sc.width)
    ext, _keep = make_ext(scene_ptr, center1, lens)
    if ext is not None:
        rc = lib(abi).rt_oracle_accumulate_ext(scene_ptr, C.byref(tiles) if tiles is not None else None, x0, x1, int(begin), int(count),
                                               C.byref(ext), accum.ctypes.data, C.byref(st), n_threads)
        if rc != 0:
            raise RuntimeError(f"rt_oracle_accumulate_ext failed: {rc}")
        return accum, st.as_dict()
    rc = lib(abi).rt_oracle_accumulate(scene_ptr, C.byref(tiles) if tiles is not None else None, x0, x1, int(begin), int(count),
                                       accum.ctypes.data, C.byref(st), n_threads)
    if rc != 0:
        raise RuntimeError(f"rt_oracle_accumulate failed: {rc}")
    return accum, st.as_dict()


def camera_ray(abi, scene_ptr, x, y, s, center1=None, lens=None):
    """rt_oracle_camera_ray_ext -> (origin (3 floats), direction (3 floats), tau) of sample s of pixel (x, y)"""
    ext, _keep = make_ext(scene_ptr, center1, lens)
    out = (C.c_double * 7)()
    rc = lib(abi).rt_oracle_camera_ray_ext(scene_ptr, C.byref(ext) if ext is not None else None, int(x), int(y), int(s), out)
    if rc != 0:
        raise RuntimeError(f"rt_oracle_camera_ray_ext failed: {rc}")
    return tuple(out[0:3]), tuple(out[3:6]), out[6]
