"""librt_hip.so — the gfx950 megakernel behind the C ABI (include/rt_abi.h), via ctypes.

This module is the product's only compute path.  It raises ImportError when the HIP library
has not been built and RtError(RT_ERR_NO_DEVICE) when no GPU is visible: there is no CPU
fallback, by design.  torch is used by callers only to own device buffers and streams; this
module passes raw device pointers.
"""
import ctypes as C
import os

from . import abi
from .host import RtError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_PROBE = None
LIB_PATH = os.path.join(_HERE, "librt_hip.so")
PROBE_LIB_PATH = os.path.join(_HERE, "librt_hip_probe.so")   # the same sources + the device probes / debug calls of include/rt_abi_test.h (tests, tools/diag.py)


def _bind(path, probes):
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing — build it with __graft_entry__.build(); "
                          "there is no CPU fallback for the hot path")
    L = C.CDLL(path)
    if os.environ.get("RT_SKIP_LAYOUT_CHECK"):   # (development: an older library for A/B runs — symbols it lacks bind to a stub)
        class _Tolerant:
            def __init__(self, lib):
                object.__setattr__(self, "_lib", lib)

            def __getattr__(self, name):
                try:
                    return getattr(self._lib, name)
                except AttributeError:
                    class _Stub:
                        argtypes = restype = None
                    return _Stub()
        L = _Tolerant(L)
    L.rt_hip_device_count.restype = C.c_int
    L.rt_hip_device_warm.argtypes = [C.c_int]
    L.rt_hip_last_error.restype = C.c_char_p
    L.rt_hip_setup_profile.restype = C.c_char_p
    L.rt_strerror.argtypes = [C.c_int]
    L.rt_strerror.restype = C.c_char_p
    L.rt_hip_scene_create.argtypes = [C.POINTER(abi.RtScene), C.c_int, C.POINTER(C.c_void_p)]
    L.rt_hip_scene_create_moving.argtypes = [C.POINTER(abi.RtScene), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_void_p)]
    L.rt_hip_scene_create_quads.argtypes = [C.POINTER(abi.RtScene), C.POINTER(C.c_double), C.POINTER(abi.RtQuad), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.rt_hip_scene_create_flats_bvh.argtypes = L.rt_hip_scene_create_quads.argtypes
    L.rt_hip_scene_destroy.argtypes = [C.c_void_p]
    L.rt_hip_scene_destroy.restype = None
    L.rt_hip_render.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_hip_wait.argtypes = [C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.rt_hip_scene_query.argtypes = [C.c_void_p, C.c_char_p]
    L.rt_hip_scene_query.restype = C.c_int64
    L.rt_hip_scene_update_spheres.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rt_hip_scene_update_flats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_group_update_flats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_scene_set_flat_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_group_set_flat_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_scene_set_flat_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_group_set_flat_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_scene_set_flat_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_group_set_flat_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_scene_set_flat_images.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_group_set_flat_images.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.rt_hip_scene_table.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rt_hip_group_update_spheres.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rt_render_rgb8.argtypes = [C.POINTER(abi.RtScene), C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_set_camera.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 4
    L.rt_hip_set_lens.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double]
    L.rt_hip_render_to_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_accumulate.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rt_hip_resolve.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_hip_refine_to_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_tile_grid.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.POINTER(C.c_uint32)]
    L.rt_hip_accumulate_tiles.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p]
    L.rt_hip_tile_error.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                    C.c_uint32, C.c_void_p, C.c_void_p]
    L.rt_hip_resolve_tiles.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_hip_render_adaptive_to_host.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_render_aovs.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_uint32, C.c_void_p, C.c_void_p]
    L.rt_hip_denoise.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_hip_refine_to_host_denoised.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_reproject.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_double)] + [C.c_float] * 5 + [C.c_void_p, C.c_void_p]
    L.rt_hip_render_frame_temporal_to_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_temporal_configure.argtypes = [C.c_void_p] + [C.c_float] * 5
    L.rt_hip_temporal_reset.argtypes = [C.c_void_p]
    L.rt_hip_temporal_history.argtypes = [C.c_void_p, C.c_void_p]
    L.rt_hip_render_surface.argtypes = [C.c_void_p, C.POINTER(abi.RtRowTiles), C.c_void_p, C.c_void_p]
    L.rt_hip_reproject_surface.argtypes = [C.c_void_p] * 7 + [C.POINTER(C.c_double), C.c_void_p] + [C.c_float] * 6 + [C.c_void_p, C.c_void_p]
    L.rt_hip_temporal_surface.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.rt_abi_sizeof.argtypes = [C.c_char_p]
    L.rt_abi_sizeof.restype = C.c_size_t
    L.rt_abi_version.restype = C.c_uint32
    L.rt_hip_group_create.argtypes = [C.POINTER(abi.RtScene), C.c_uint32, C.POINTER(C.c_void_p)]
    L.rt_hip_group_create_moving.argtypes = [C.POINTER(abi.RtScene), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_void_p)]
    L.rt_hip_group_create_quads.argtypes = [C.POINTER(abi.RtScene), C.POINTER(C.c_double), C.POINTER(abi.RtQuad), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.rt_hip_group_create_flats_bvh.argtypes = L.rt_hip_group_create_quads.argtypes
    L.rt_hip_group_destroy.argtypes = [C.c_void_p]
    L.rt_hip_group_destroy.restype = None
    L.rt_hip_group_size.argtypes = [C.c_void_p]
    L.rt_hip_group_size.restype = C.c_uint32
    L.rt_hip_group_set_camera.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 4
    L.rt_hip_group_set_lens.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double]
    L.rt_hip_group_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.rt_hip_group_render_to_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_group_render.argtypes = [C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_group_submit.argtypes = [C.c_void_p, C.c_void_p]
    L.rt_hip_group_collect.argtypes = [C.c_void_p, C.POINTER(abi.RtStats)]
    L.rt_hip_group_info.argtypes = [C.c_void_p, C.POINTER(abi.RtGroupInfo)]
    L.rt_hip_group_ranks.argtypes = [C.c_void_p, C.POINTER(abi.RtGroupRank), C.c_uint32]
    L.rt_hip_group_ranks.restype = C.c_uint32
    L.rt_hip_group_fallback_reason.argtypes = [C.c_void_p]
    L.rt_hip_group_fallback_reason.restype = C.c_char_p
    L.rt_hip_group_frame.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.rt_hip_group_frame.restype = C.c_void_p
    L.rt_hip_group_stacked_row.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rt_hip_group_stacked_row.restype = C.c_uint32
    if probes:   # include/rt_abi_test.h
        L.rt_hip_debug_timeline.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_hip_debug_tile_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rt_hip_math_probe.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p]
        L.rt_hip_hit_probe.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
        L.rt_hip_atan2_probe.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
        L.rt_hip_texel_probe.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_hip_quot_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
        L.rt_hip_render_rays_probe.argtypes = [C.c_void_p] * 6 + [C.POINTER(abi.RtStats)]
        L.rt_hip_walk_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
        L.rt_hip_quad_probe.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 3 + [C.c_void_p] * 6
        L.rt_hip_neg_log_probe.argtypes = [C.c_void_p] * 2 + [C.c_uint32, C.c_void_p]
        L.rt_hip_solid_fn_probe.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
        L.rt_hip_solid_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_hip_medium_probe.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p]
        L.rt_hip_flat_shutter_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 2 + [C.c_void_p] * 7   # include/rt_abi_test_flat_motion.h
    for name in (() if os.environ.get("RT_SKIP_LAYOUT_CHECK") else ("RtSphere", "RtQuad", "RtTexture", "RtScene", "RtRowTiles", "RtStats", "RtGroupInfo", "RtGroupRank")):   # the binding's own layout check
        if L.rt_abi_sizeof(name.encode()) != C.sizeof(getattr(abi, name)):
            raise ImportError(f"{path}: sizeof({name}) = {L.rt_abi_sizeof(name.encode())} but abi.py has "
                              f"{C.sizeof(getattr(abi, name))} — rebuild with __graft_entry__.build()")
    if L.rt_abi_version() != abi.RT_ABI_VERSION and not os.environ.get("RT_SKIP_LAYOUT_CHECK"):
        raise ImportError(f"{path}: ABI version {L.rt_abi_version()} != {abi.RT_ABI_VERSION}")
    return L


def lib():
    """the PRODUCT library (include/rt_abi.h)"""
    global _LIB
    if _LIB is None:
        _LIB = _bind(LIB_PATH, probes=False)
    return _LIB


def probe_lib():
    """librt_hip_probe.so: the product's sources + the device probes and debug calls of include/rt_abi_test.h — test
    infrastructure.  A scene the debug calls look into must have been created through THIS library: HipScene(..., library=probe_lib())."""
    global _PROBE
    if _PROBE is None:
        _PROBE = _bind(PROBE_LIB_PATH, probes=True)
    return _PROBE


def _check(rc, L=None):
    if rc != abi.RT_OK:
        L = L or lib()
        raise RtError(rc, f"{L.rt_strerror(rc).decode()}: {L.rt_hip_last_error().decode('utf-8', 'replace')}")


def setup_profile():
    """rt_hip_setup_profile: {stage: ms} of the most recent group creation / one-shot render of this process"""
    import json
    return json.loads(lib().rt_hip_setup_profile().decode())


def device_count():
    return lib().rt_hip_device_count()


def _center1_array(scene_ptr, center1):
    """n_spheres x 3 centres at shutter close as the C array rt_hip_*_create_moving read"""
    n = scene_ptr.contents.n_spheres
    flat = [float(x) for c in center1 for x in c]
    if len(flat) != 3 * n:
        raise ValueError(f"center1 needs {n} x 3 values, got {len(flat)}")
    return (C.c_double * max(1, 3 * n))(*flat)


def _centres(n, c, what):
    """n x 3 centres (anything numpy can flatten) as a C array of doubles; None stays None"""
    import numpy as np
    if c is None:
        return None
    a = np.ascontiguousarray(np.asarray(c, np.float64).reshape(-1))
    if a.size != 3 * n:
        raise ValueError(f"{what} needs {n} x 3 values, got {a.size}")
    return (C.c_double * max(1, 3 * n)).from_buffer_copy(a.tobytes() if n else bytes(8))


def _flat_geometry(quv, device, rebuild, width=9, what="quv", dtype="float64"):
    """the arguments of rt_hip_*_update_flats for quv, an [n, 9] float64 numpy array (or anything numpy makes one of) or a CUDA torch
    tensor of that shape and dtype: (pointer, n, flags, what must stay alive over the call).  A contiguous tensor on `device` (an index;
    None: never) is handed over as device memory; any other tensor travels through the host."""
    import numpy as np
    flags = abi.RT_UPDATE_FLATS_REBUILD if rebuild else 0
    if hasattr(quv, "data_ptr") and hasattr(quv, "is_cuda"):   # a torch tensor
        if quv.dim() != 2 or quv.shape[1] != width or str(quv.dtype) != "torch." + dtype:
            raise ValueError(f"{what} must be an [n, {width}] {dtype} tensor, got {tuple(quv.shape)} {quv.dtype}")
        if quv.is_cuda and quv.is_contiguous() and device is not None and quv.device.index == device:
            import torch
            torch.cuda.current_stream(quv.device).synchronize()   # (the library reads on its own stream: what wrote the tensor has finished)
            return C.c_void_p(quv.data_ptr()), quv.shape[0], flags | abi.RT_UPDATE_FLATS_DEVICE, quv
        quv = quv.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(quv, np.dtype(dtype)))
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what} must be n x {width} values, got shape {a.shape}")
    return C.c_void_p(a.ctypes.data), a.shape[0], flags, a


def _flat_images(images, device):
    """the arguments of rt_hip_*_set_flat_images: a sequence (or ctypes array) of abi.RtFlatImage, an [n, 64] uint8 numpy array of such
    records, or an [n, 64] uint8 CUDA torch tensor — contiguous and on `device` it is read where it is: (pointer, n, flags, keep alive)"""
    import numpy as np
    size = C.sizeof(abi.RtFlatImage)
    if hasattr(images, "data_ptr") and hasattr(images, "is_cuda"):   # a torch tensor
        if images.dim() != 2 or images.shape[1] != size or str(images.dtype) != "torch.uint8":
            raise ValueError(f"images must be an [n, {size}] uint8 tensor, got {tuple(images.shape)} {images.dtype}")
        if images.is_cuda and images.is_contiguous() and device is not None and images.device.index == device:
            import torch
            torch.cuda.current_stream(images.device).synchronize()
            return C.c_void_p(images.data_ptr()), images.shape[0], abi.RT_UPDATE_FLATS_DEVICE, images
        images = images.detach().cpu().numpy()
    if isinstance(images, np.ndarray):
        a = np.ascontiguousarray(images, np.uint8)
        if a.ndim != 2 or a.shape[1] != size:
            raise ValueError(f"images must be n x {size} bytes, got shape {a.shape}")
        return C.c_void_p(a.ctypes.data), a.shape[0], 0, a
    n = len(images)
    if isinstance(images, C.Array) and images._type_ is abi.RtFlatImage:
        return C.cast(images, C.c_void_p), n, 0, images
    arr = (abi.RtFlatImage * max(1, n))()
    for i, x in enumerate(images):
        arr[i] = x
    return C.cast(arr, C.c_void_p), n, 0, arr


def _flat_call(L, name, handle, args):
    """one call of rt_hip_{scene,group}_update_flats or ..._set_flat_*: args is what _flat_geometry, _flat_images or _flat_none gave —
    (pointer, n, flags, what must stay alive until the call has returned)"""
    p, n, flags, keep = args
    _check(getattr(L, name)(handle, p, n, flags), L)
    del keep


def _flat_none(n_quads):
    """the arguments that remove a table: a null pointer and the scene's count"""
    return None, int(n_quads), 0, None


TABLES = ("grid", "cell_word", "cell_items", "large", "geom", "large_geom", "motion", "quads", "quad_lim", "flat_bvh", "flat_bvh_order", "flat_normals", "flat_motion", "flat_lights", "flat_images", "lights", "mat", "matc")   # the names rt_hip_scene_table knows


def _quads_array(quads):
    """a sequence of abi.RtQuad (or a ctypes array of them) as (C array, count)"""
    n = len(quads)
    if isinstance(quads, C.Array) and quads._type_ is abi.RtQuad:
        return quads, n
    arr = (abi.RtQuad * max(1, n))()
    for i, q in enumerate(quads):
        arr[i] = q
    return arr, n


# bits of query("last_kernel") (include/rt_abi.h rt_hip_scene_query)
KERNEL_LDS, KERNEL_SIMPLE, KERNEL_LIGHTS, KERNEL_WIDE, KERNEL_ACCUM, KERNEL_LENS, KERNEL_MOTION, KERNEL_MEDIUM, KERNEL_SOLID, KERNEL_QUADS = (1 << b for b in range(10))


class HipScene:
    """Scene tables + textures resident in HBM of one GPU (rt_hip_scene_create).  `library`: probe_lib() for the tests and
    tools that use the debug calls; default: the product library."""

    def __init__(self, scene_ptr, device=0, library=None, center1=None, quads=None, flat_bvh=False):
        """center1 (motion blur): None, or each sphere's centre at shutter close, n_spheres x 3 (host.Scene.center1()):
        rt_hip_scene_create_moving.  quads: None, or the scene's flat primitives, abi.RtQuad records whose `reserved` is abi.RT_QUAD_SHAPE_* (host.Scene.quads()):
        rt_hip_scene_create_quads; flat_bvh: with the structure over them, rt_hip_scene_create_flats_bvh (it needs quads)"""
        self._L = library or lib()
        self._h = C.c_void_p()
        if flat_bvh and quads is None:
            raise ValueError("flat_bvh needs quads")
        if quads is not None:
            qa, nq = _quads_array(quads)
            c1 = _center1_array(scene_ptr, center1) if center1 is not None else None
            create = self._L.rt_hip_scene_create_flats_bvh if flat_bvh else self._L.rt_hip_scene_create_quads
            _check(create(scene_ptr, c1, qa, nq, device, C.byref(self._h)), self._L)
        elif center1 is None:
            _check(self._L.rt_hip_scene_create(scene_ptr, device, C.byref(self._h)), self._L)
        else:
            c1 = _center1_array(scene_ptr, center1)
            _check(self._L.rt_hip_scene_create_moving(scene_ptr, c1, device, C.byref(self._h)), self._L)
        sc = scene_ptr.contents
        self.width, self.height = sc.width, sc.height
        self.device = device
        self.n_spheres = sc.n_spheres

    def update_spheres(self, center, center1=None):
        """rt_hip_scene_update_spheres: move the spheres to `center` (n_spheres x 3, shutter open) and `center1` (None, or
        n_spheres x 3 at shutter close); the grid is rebuilt on the device.  Blocking."""
        _check(self._L.rt_hip_scene_update_spheres(self._h, _centres(self.n_spheres, center, "center"), _centres(self.n_spheres, center1, "center1")),
               self._L)

    def update_flats(self, quv, rebuild=False):
        """rt_hip_scene_update_flats: move the flat primitives to quv — [n_quads, 9] float64 (q, u, v per entry), a numpy
        array or a CUDA torch tensor; a contiguous tensor on the scene's device is read where it is (no PCIe).  The structure is refit on
        the device; rebuild=True (or a change of the set of entries outside its preconditions) builds it anew: on the host, or with
        set_option("flat_build", 1) and an unchanged set on the device.  Blocking."""
        _flat_call(self._L, "rt_hip_scene_update_flats", self._h, _flat_geometry(quv, self.device, rebuild))

    def set_flat_normals(self, normals):
        """rt_hip_scene_set_flat_normals: shading normals on the scene's triangles — [n_quads, 9] float64 (the normals at q,
        q + u, q + v per entry; nine zeros: a flat entry), a numpy array or a CUDA torch tensor as for update_flats; None removes them.
        Blocking."""
        _flat_call(self._L, "rt_hip_scene_set_flat_normals", self._h, _flat_none(self.query("quads")) if normals is None else _flat_geometry(normals, self.device, False))

    def set_flat_motion(self, move):
        """rt_hip_scene_set_flat_motion: the displacement of every flat primitive over the open shutter — [n_quads, 3]
        float64 (three zeros: the entry does not move), a numpy array or a CUDA torch tensor as for update_flats; None removes the
        motion.  Blocking."""
        _flat_call(self._L, "rt_hip_scene_set_flat_motion", self._h, _flat_none(self.query("quads")) if move is None else _flat_geometry(move, self.device, False, width=3, what="move"))

    def set_flat_lights(self, emit):
        """rt_hip_scene_set_flat_lights: the emission of every flat primitive — [n_quads, 3] float32 in [0, 1] (three
        zeros: the entry does not emit), a numpy array or a CUDA torch tensor as for update_flats; None removes emission.  Blocking."""
        _flat_call(self._L, "rt_hip_scene_set_flat_lights", self._h, _flat_none(self.query("quads")) if emit is None else _flat_geometry(emit, self.device, False, width=3, what="emit", dtype="float32"))

    def set_flat_images(self, images):
        """rt_hip_scene_set_flat_images: the image of every flat primitive — n_quads abi.RtFlatImage (abi.flat_image(...);
        tex_id abi.RT_FLAT_IMAGE_NONE: the entry has none) as a sequence, an [n, 64] uint8 numpy array or a CUDA torch tensor of that
        shape (read where it is when on the scene's device); None removes the images.  Blocking."""
        _flat_call(self._L, "rt_hip_scene_set_flat_images", self._h, _flat_none(self.query("quads")) if images is None else _flat_images(images, self.device))

    def table(self, name):
        """rt_hip_scene_table (diagnostics): the bytes of one resident table (TABLES) as the kernels read it"""
        need = C.c_size_t(0)
        _check(self._L.rt_hip_scene_table(self._h, name.encode(), None, 0, C.byref(need)), self._L)
        buf = C.create_string_buffer(max(1, need.value))
        _check(self._L.rt_hip_scene_table(self._h, name.encode(), buf, need.value, C.byref(need)), self._L)
        return buf.raw[:need.value]

    def set_option(self, key, value):
        _check(self._L.rt_hip_set_option(self._h, key.encode(), int(value)), self._L)

    def query(self, key):
        """rt_hip_scene_query: what the resident scene was built into ("grid_cells", "table_bytes", "media", "solids", ...) and
        "last_kernel", the instantiation that ran (KERNEL_* bits below); -1 = unknown key"""
        return int(self._L.rt_hip_scene_query(self._h, key.encode()))

    def render(self, d_rgb8, d_linear=0, tiles=None, stream=0):
        """enqueue the megakernel; d_* are raw device pointers (ints), stream a hipStream_t"""
        _check(self._L.rt_hip_render(self._h, C.byref(tiles) if tiles is not None else None,
                                     C.c_void_p(d_rgb8), C.c_void_p(d_linear or None), C.c_void_p(stream or None)), self._L)

    def set_camera(self, origin, lower_left, horizontal, vertical):
        """move the camera of the resident scene (the four vectors of camera.rs:52-63)"""
        v = [(C.c_double * 3)(*x) for x in (origin, lower_left, horizontal, vertical)]
        _check(self._L.rt_hip_set_camera(self._h, *v), self._L)

    def set_lens(self, u, v, lens_radius):
        """thin-lens camera: the unit vectors u, v of the lens plane and its radius; 0 = the pinhole"""
        _check(self._L.rt_hip_set_lens(self._h, (C.c_double * 3)(*u), (C.c_double * 3)(*v), float(lens_radius)), self._L)

    def render_to_host(self):
        """whole frame into a numpy [h,w,3] array (blocking) + stats"""
        import numpy as np
        out = np.zeros((self.height, self.width, 3), np.uint8)
        st = abi.RtStats()
        _check(self._L.rt_hip_render_to_host(self._h, out.ctypes.data, C.byref(st)), self._L)
        return out, st.as_dict()

    def accumulate(self, d_accum, sample_begin, sample_count, tiles=None, stream=0):
        """enqueue samples [sample_begin, sample_begin + sample_count) of every pixel of `tiles`, their exact fixed-point sums
        ADDED to d_accum (a zeroed device buffer of rows x width x 3 uint64, 8-byte aligned; include/rt_abi.h); wait() reports it"""
        _check(self._L.rt_hip_accumulate(self._h, C.byref(tiles) if tiles is not None else None, int(sample_begin), int(sample_count),
                                         C.c_void_p(d_accum or None), C.c_void_p(stream or None)), self._L)

    def resolve(self, d_accum, n_samples, d_rgb8, d_linear=0, tiles=None, stream=0):
        """enqueue the resolve of d_accum holding n_samples samples per pixel into d_rgb8 / d_linear (either may be 0)"""
        _check(self._L.rt_hip_resolve(self._h, C.byref(tiles) if tiles is not None else None, C.c_void_p(d_accum or None), int(n_samples),
                                      C.c_void_p(d_rgb8 or None), C.c_void_p(d_linear or None), C.c_void_p(stream or None)), self._L)

    def refine_to_host(self, sample_count):
        """the next sample_count samples into the scene's own accumulator; the frame resolved over all it holds as a numpy
        [h,w,3] array (blocking) + the pass's stats.  query("accum_samples") says how many samples per pixel it holds."""
        import numpy as np
        out = np.zeros((self.height, self.width, 3), np.uint8)
        st = abi.RtStats()
        _check(self._L.rt_hip_refine_to_host(self._h, int(sample_count), out.ctypes.data, C.byref(st)), self._L)
        return out, st.as_dict()

    # include/rt_abi.h RT_DENOISE_*: the defaults of the host form and the CLI's --denoise
    DENOISE_ITERATIONS = 2
    DENOISE_SIGMAS = (0.25, 0.1, 0.1, 0.01)   # colour, normal, albedo, inv_depth
    DENOISE_AOV_SAMPLES = 8

    def render_aovs(self, n_samples, d_aov, tiles=None, stream=0):
        """enqueue the feature buffers of samples [0, n_samples): per pixel 8 float32 {albedo rgb, inv_depth, normal xyz, coverage}
        into d_aov (height x width x 8 float32, 16-byte aligned); whole frames only (tiles must be None)"""
        _check(self._L.rt_hip_render_aovs(self._h, C.byref(tiles) if tiles is not None else None, int(n_samples), C.c_void_p(d_aov or None),
                                          C.c_void_p(stream or None)), self._L)

    def denoise(self, d_linear, d_aov, iterations=DENOISE_ITERATIONS, d_out_linear=0, d_out_rgb8=0, sigmas=DENOISE_SIGMAS, tiles=None, stream=0):
        """enqueue `iterations` passes of the a-trous filter over d_linear (height x width x 3 float32) guided by d_aov, into
        d_out_linear and / or d_out_rgb8 (either may be 0); sigmas = (colour, normal, albedo, inv_depth)"""
        sc, sn, sa, sz = (float(x) for x in sigmas)
        _check(self._L.rt_hip_denoise(self._h, C.byref(tiles) if tiles is not None else None, C.c_void_p(d_linear or None), C.c_void_p(d_aov or None),
                                      int(iterations), sc, sn, sa, sz, C.c_void_p(d_out_linear or None), C.c_void_p(d_out_rgb8 or None),
                                      C.c_void_p(stream or None)), self._L)

    def refine_to_host_denoised(self, sample_count, iterations=DENOISE_ITERATIONS):
        """refine_to_host() with the frame denoised (default sigmas) before it leaves: numpy [h,w,3] uint8 + the pass's stats"""
        import numpy as np
        out = np.zeros((self.height, self.width, 3), np.uint8)
        st = abi.RtStats()
        _check(self._L.rt_hip_refine_to_host_denoised(self._h, int(sample_count), int(iterations), out.ctypes.data, C.byref(st)), self._L)
        return out, st.as_dict()

    # include/rt_abi.h RT_TEMPORAL_*: alpha_min, n_max, tau_n, tau_a, tau_z a scene starts with (the best of a sweep)
    TEMPORAL_PARAMS = (0.5, 8.0, 0.02, 0.3, 0.02)

    def reproject(self, d_linear, d_aov, d_prev_history, d_prev_aov, prev_camera, d_out_history, params=TEMPORAL_PARAMS, stream=0):
        """enqueue one temporal step: this frame's d_linear (h x w x 3 float32) and d_aov blended with the previous
        frame's d_prev_history (h x w x 4 float32 {r, g, b, n}) found through d_prev_aov and prev_camera (12 doubles: origin, lower_left,
        horizontal, vertical) into d_out_history; params = (alpha_min, n_max, tau_n, tau_a, tau_z)"""
        cam = (C.c_double * 12)(*[float(x) for x in prev_camera]) if prev_camera is not None else None
        _check(self._L.rt_hip_reproject(self._h, C.c_void_p(d_linear or None), C.c_void_p(d_aov or None), C.c_void_p(d_prev_history or None),
                                        C.c_void_p(d_prev_aov or None), cam, *[float(x) for x in params], C.c_void_p(d_out_history or None),
                                        C.c_void_p(stream or None)), self._L)

    def render_frame_temporal_to_host(self, frame_index, iterations=DENOISE_ITERATIONS):
        """frame `frame_index` of an animation: its own sample range, reprojected onto the history the previous call left, filtered:
        numpy [h,w,3] uint8 + the pass's stats (blocking)"""
        import numpy as np
        out = np.zeros((self.height, self.width, 3), np.uint8)
        st = abi.RtStats()
        _check(self._L.rt_hip_render_frame_temporal_to_host(self._h, int(frame_index), int(iterations), out.ctypes.data, C.byref(st)), self._L)
        return out, st.as_dict()

    def temporal_configure(self, alpha_min, n_max, tau_n, tau_a, tau_z):
        _check(self._L.rt_hip_temporal_configure(self._h, float(alpha_min), float(n_max), float(tau_n), float(tau_a), float(tau_z)), self._L)

    def temporal_reset(self):
        _check(self._L.rt_hip_temporal_reset(self._h), self._L)

    def temporal_history(self):
        """the history the last temporal frame left: numpy [h,w,4] float32 {r, g, b, n}"""
        import numpy as np
        out = np.zeros((self.height, self.width, 4), np.float32)
        _check(self._L.rt_hip_temporal_history(self._h, out.ctypes.data), self._L)
        return out

    # include/rt_abi.h RT_TEMPORAL_SURFACE_*: alpha_min, alpha_specular the CLI's --temporal-surface configures (the best of a sweep)
    TEMPORAL_SURFACE_PARAMS = (0.5, 1.0)

    def render_surface(self, d_surface, tiles=None, stream=0):
        """enqueue the surface record of every pixel: 16 bytes {uint32 id, uint32 kind, float64 t} of what the
        pixel-centre pinhole ray meets first (id = kind = 0xFFFFFFFF, t = 0: the sky) into d_surface (height x width x 16 bytes,
        16-byte aligned); whole frames only (tiles must be None)"""
        _check(self._L.rt_hip_render_surface(self._h, C.byref(tiles) if tiles is not None else None, C.c_void_p(d_surface or None),
                                             C.c_void_p(stream or None)), self._L)

    def reproject_surface(self, d_linear, d_aov, d_surface, d_prev_history, d_prev_aov, d_prev_surface, prev_camera, d_out_history, d_displacement=0,
                          params=TEMPORAL_PARAMS, alpha_specular=TEMPORAL_SURFACE_PARAMS[1], stream=0):
        """enqueue one temporal step with surface tracking: reproject() with the two frames' surface records and d_displacement (0, or
        n_spheres x 3 float64 on the device: each sphere's centre now minus its centre one frame ago); params = (alpha_min, n_max, tau_n,
        tau_a, tau_z), alpha_specular = the floor on alpha of Metal and Glass pixels"""
        cam = (C.c_double * 12)(*[float(x) for x in prev_camera]) if prev_camera is not None else None
        a_min, n_max, tau_n, tau_a, tau_z = (float(x) for x in params)
        _check(self._L.rt_hip_reproject_surface(self._h, C.c_void_p(d_linear or None), C.c_void_p(d_aov or None), C.c_void_p(d_surface or None),
                                                C.c_void_p(d_prev_history or None), C.c_void_p(d_prev_aov or None), C.c_void_p(d_prev_surface or None),
                                                cam, C.c_void_p(d_displacement or None), a_min, float(alpha_specular), n_max, tau_n, tau_a, tau_z,
                                                C.c_void_p(d_out_history or None), C.c_void_p(stream or None)), self._L)

    def temporal_surface(self, enable, alpha_specular=TEMPORAL_SURFACE_PARAMS[1]):
        """render_frame_temporal_to_host() with (True) or without (False, how a scene starts) surface tracking; a change of mode drops
        the history.  temporal_configure() supplies the other five values in both modes."""
        _check(self._L.rt_hip_temporal_surface(self._h, 1 if enable else 0, float(alpha_specular)), self._L)

    def tile_grid(self, tiles=None):
        """the pixel tiles of adaptive sampling for `tiles`' rows: (tile width, tile height, tiles_x, tiles_y); id = ty * tiles_x + tx"""
        out = (C.c_uint32 * 4)()
        _check(self._L.rt_hip_tile_grid(self._h, C.byref(tiles) if tiles is not None else None, out), self._L)
        return tuple(int(v) for v in out)

    def accumulate_tiles(self, d_list, n_list, d_accum, sample_begin, sample_count, tiles=None, stream=0):
        """accumulate() for just the n_list distinct tile ids of d_list (device uint32; ids past the grid are skipped)"""
        _check(self._L.rt_hip_accumulate_tiles(self._h, C.byref(tiles) if tiles is not None else None, C.c_void_p(d_list or None), int(n_list),
                                               int(sample_begin), int(sample_count), C.c_void_p(d_accum or None), C.c_void_p(stream or None)), self._L)

    def tile_error(self, d_list, n_list, d_now, n_now, d_prev, n_prev, d_tile_err, tiles=None, stream=0):
        """enqueue the noise estimate of the listed tiles (d_now: samples [0, n_now), d_prev: [0, n_prev)) into d_tile_err[id] (float64)"""
        _check(self._L.rt_hip_tile_error(self._h, C.byref(tiles) if tiles is not None else None, C.c_void_p(d_list or None), int(n_list),
                                         C.c_void_p(d_now or None), int(n_now), C.c_void_p(d_prev or None), int(n_prev),
                                         C.c_void_p(d_tile_err or None), C.c_void_p(stream or None)), self._L)

    def resolve_tiles(self, d_accum, d_tile_spp, d_rgb8, d_linear=0, tiles=None, stream=0):
        """enqueue resolve() with each pixel over its tile's count d_tile_spp[id] (device uint32, tiles_y x tiles_x)"""
        _check(self._L.rt_hip_resolve_tiles(self._h, C.byref(tiles) if tiles is not None else None, C.c_void_p(d_accum or None),
                                            C.c_void_p(d_tile_spp or None), C.c_void_p(d_rgb8 or None), C.c_void_p(d_linear or None),
                                            C.c_void_p(stream or None)), self._L)

    def render_adaptive(self, threshold, min_spp=16):
        """one adaptive frame (blocking): rgb8 numpy [h,w,3], the per-tile counts [tiles_y, tiles_x] and the frame's stats"""
        import numpy as np
        _, _, tx, ty = self.tile_grid()
        out = np.zeros((self.height, self.width, 3), np.uint8)
        spp = np.zeros((ty, tx), np.uint32)
        st = abi.RtStats()
        _check(self._L.rt_hip_render_adaptive_to_host(self._h, float(threshold), int(min_spp), out.ctypes.data, spp.ctypes.data, C.byref(st)),
               self._L)
        return out, spp, st.as_dict()

    def adaptive_rounds(self):
        """the rounds of the last render_adaptive: [(tiles, samples per pixel after the round, kernel ms)]"""
        return [(self.query(f"adaptive_round_tiles_{i}"), self.query(f"adaptive_round_spp_{i}"), self.query(f"adaptive_round_kernel_us_{i}") / 1000.0)
                for i in range(max(self.query("adaptive_rounds"), 0))]

    def wait(self):
        st = abi.RtStats()
        _check(self._L.rt_hip_wait(self._h, C.byref(st)), self._L)
        return st.as_dict()

    def debug_tile_depth(self, cap=1 << 22):
        """(probe library only) deepest camera path per pixel tile of the last measuring frame, as a 2-D array [tile rows, tile columns]"""
        import numpy as np
        buf = np.zeros(cap, np.uint32)
        tx = C.c_uint32(0)
        n = self._L.rt_hip_debug_tile_depth(self._h, buf.ctypes.data, cap, C.byref(tx))
        if n < 0:
            _check(n, self._L)
        return buf[:n].reshape(-1, tx.value) if tx.value and n % tx.value == 0 else buf[:n]

    def debug_timeline(self, max_waves=8192):
        """(probe library only) {start, end, queue-empty time, tail iterations | lane-iterations << 32} of every wave of the last launch, 100 MHz ticks (RT_PROFILE builds of the library only)."""
        import numpy as np
        buf = np.zeros(32 + 4 * max_waves, np.uint64)
        n = self._L.rt_hip_debug_timeline(self._h, buf.ctypes.data, max_waves)
        if n < 0:
            _check(n, self._L)
        return buf[32:32 + 4 * n].reshape(n, 4), buf[:32]

    def render_rays_probe(self, d_rays, d_rgb8, d_linear=0, d_first_t=0, d_first_sphere=0):
        """(probe library only) rt_hip_render_rays_probe: one frame whose camera rays are d_rays (h x w x 6 f64 on the device),
        waited for -> stats dict"""
        st = abi.RtStats()
        _check(self._L.rt_hip_render_rays_probe(self._h, C.c_void_p(d_rays), C.c_void_p(d_first_t or None), C.c_void_p(d_first_sphere or None),
                                                C.c_void_p(d_rgb8), C.c_void_p(d_linear or None), C.byref(st)), self._L)
        return st.as_dict()

    def walk_probe(self, d_rays, d_t, d_best, n, d_work=0, stream=0):
        """(probe library only) rt_hip_walk_probe: hit_world_grid of n rays (device pointers; d_work: n x 2 u32 exact tests, grid
        steps), enqueued on `stream`"""
        _check(self._L.rt_hip_walk_probe(self._h, C.c_void_p(d_rays), C.c_void_p(d_t), C.c_void_p(d_best), C.c_void_p(d_work or None), n,
                                         C.c_void_p(stream or None)), self._L)

    def quad_probe(self, d_rays, d_closest, n, first_quad, n_quads, d_best, d_t, d_point, d_normal, d_front, stream=0):
        """(probe library only) rt_hip_quad_probe: quads_hit of n rays with their own closest-so-far against the scene's quads first_quad ..
        first_quad + n_quads - 1, then object_surface of the accepted id (device pointers), enqueued on `stream`"""
        _check(self._L.rt_hip_quad_probe(self._h, C.c_void_p(d_rays), C.c_void_p(d_closest), n, first_quad, n_quads, C.c_void_p(d_best), C.c_void_p(d_t),
                                         C.c_void_p(d_point), C.c_void_p(d_normal), C.c_void_p(d_front), C.c_void_p(stream or None)), self._L)

    def solid_probe(self, sphere, d_points, d_rgb, n, stream=0):
        """(probe library only) rt_hip_solid_probe: solid_albedo of n world-space points (n x 3 f64) on the Checker or Noise sphere `sphere`
        -> d_rgb (n x 3 f32; device pointers), enqueued on `stream`"""
        _check(self._L.rt_hip_solid_probe(self._h, sphere, C.c_void_p(d_points), C.c_void_p(d_rgb), n, C.c_void_p(stream or None)), self._L)

    def medium_probe(self, d_rays, d_node, d_t, d_best, n, d_tau=0, d_work=0, stream=0):
        """(probe library only) rt_hip_medium_probe: hit_world with the medium candidate of n rays, ray i at the RNG address (pixel i, sample
        0, d_node[i]) and shutter time d_tau[i] (f32; 0: time 0) -> d_t, d_best, d_work (optional, n x 2 u32; device pointers), enqueued on
        `stream`"""
        _check(self._L.rt_hip_medium_probe(self._h, C.c_void_p(d_rays), C.c_void_p(d_tau or None), C.c_void_p(d_node), C.c_void_p(d_t), C.c_void_p(d_best),
                                           C.c_void_p(d_work or None), n, C.c_void_p(stream or None)), self._L)

    def flat_shutter_probe(self, d_rays, d_closest, n, d_best, d_t, d_point, d_normal, d_front, d_origin, d_tau=0, d_best_in=0, block=192, stream=0):
        """(probe library only) rt_hip_flat_shutter_probe (include/rt_abi_test_flat_motion.h): flats_hit of n rays through the motion tables
        at shutter time d_tau[i] (f32; 0: time 0), each with its closest-so-far and the hit it holds (d_best_in, i32; 0: -1), then
        object_surface<true> of a newly accepted flat entry -> d_best always, d_t, d_point, d_normal, d_front, d_origin on such a hit
        (device pointers), in workgroups of `block`, enqueued on `stream`"""
        _check(self._L.rt_hip_flat_shutter_probe(self._h, C.c_void_p(d_rays or None), C.c_void_p(d_tau or None), C.c_void_p(d_closest or None),
                                                 C.c_void_p(d_best_in or None), n, block, C.c_void_p(d_best or None), C.c_void_p(d_t or None),
                                                 C.c_void_p(d_point or None), C.c_void_p(d_normal or None), C.c_void_p(d_front or None),
                                                 C.c_void_p(d_origin or None), C.c_void_p(stream or None)), self._L)

    def close(self):
        if self._h:
            self._L.rt_hip_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipGroup:
    """The scene resident on n_gpus devices of this node, frames sharded by interleaved scanline tiles
    inside librt_hip.so (rt_hip_group_*): host threads + streams + ONE gather per frame, no torch."""

    def __init__(self, scene_ptr, n_gpus=0, library=None, center1=None, quads=None, flat_bvh=False):
        self._L = library or lib()     # (library: probe_lib() for the tests that inject transport faults)
        self._h = C.c_void_p()
        if flat_bvh and quads is None:
            raise ValueError("flat_bvh needs quads")
        if quads is not None:  # (quads, DESIGN.md §20: rt_hip_group_create_quads; flat_bvh, §22: rt_hip_group_create_flats_bvh)
            qa, nq = _quads_array(quads)
            c1 = _center1_array(scene_ptr, center1) if center1 is not None else None
            create = self._L.rt_hip_group_create_flats_bvh if flat_bvh else self._L.rt_hip_group_create_quads
            _check(create(scene_ptr, c1, qa, nq, n_gpus, C.byref(self._h)), self._L)
        elif center1 is None:
            _check(self._L.rt_hip_group_create(scene_ptr, n_gpus, C.byref(self._h)), self._L)
        else:  # (motion blur, DESIGN.md §14: rt_hip_group_create_moving)
            c1 = _center1_array(scene_ptr, center1)
            _check(self._L.rt_hip_group_create_moving(scene_ptr, c1, n_gpus, C.byref(self._h)), self._L)
        sc = scene_ptr.contents
        self.width, self.height = sc.width, sc.height
        self.size = self._L.rt_hip_group_size(self._h)
        self.n_spheres = sc.n_spheres

    def update_spheres(self, center, center1=None):
        """rt_hip_group_update_spheres: HipScene.update_spheres on every rank; no submitted frame may be uncollected"""
        _check(self._L.rt_hip_group_update_spheres(self._h, _centres(self.n_spheres, center, "center"), _centres(self.n_spheres, center1, "center1")),
               self._L)

    def update_flats(self, quv, rebuild=False):
        """rt_hip_group_update_flats: HipScene.update_flats on every rank (the geometry travels through host memory: the ranks may be on
        several devices); no submitted frame may be uncollected"""
        _flat_call(self._L, "rt_hip_group_update_flats", self._h, _flat_geometry(quv, None, rebuild))

    def set_flat_normals(self, normals, n_quads=None):
        """rt_hip_group_set_flat_normals: HipScene.set_flat_normals on every rank (through host memory); None removes them and needs
        n_quads, the scene's count"""
        _flat_call(self._L, "rt_hip_group_set_flat_normals", self._h, _flat_none(n_quads) if normals is None else _flat_geometry(normals, None, False))

    def set_flat_motion(self, move, n_quads=None):
        """rt_hip_group_set_flat_motion: HipScene.set_flat_motion on every rank (through host memory); None removes the motion and needs
        n_quads, the scene's count"""
        _flat_call(self._L, "rt_hip_group_set_flat_motion", self._h, _flat_none(self._count("set_flat_motion", n_quads)) if move is None else _flat_geometry(move, None, False, width=3, what="move"))

    def set_flat_lights(self, emit, n_quads=None):
        """rt_hip_group_set_flat_lights: HipScene.set_flat_lights on every rank (through host memory); None removes emission and needs
        n_quads, the scene's count"""
        _flat_call(self._L, "rt_hip_group_set_flat_lights", self._h, _flat_none(self._count("set_flat_lights", n_quads)) if emit is None else _flat_geometry(emit, None, False, width=3, what="emit", dtype="float32"))

    def set_flat_images(self, images, n_quads=None):
        """rt_hip_group_set_flat_images: HipScene.set_flat_images on every rank (through host memory); None removes the images and needs
        n_quads, the scene's count"""
        _flat_call(self._L, "rt_hip_group_set_flat_images", self._h, _flat_none(self._count("set_flat_images", n_quads)) if images is None else _flat_images(images, None))

    @staticmethod
    def _count(method, n_quads):
        if n_quads is None:
            raise ValueError(f"{method}(None) needs n_quads, the scene's count")
        return n_quads

    def set_option(self, key, value):
        _check(self._L.rt_hip_group_set_option(self._h, key.encode(), int(value)), self._L)

    def set_camera(self, origin, lower_left, horizontal, vertical):
        v = [(C.c_double * 3)(*x) for x in (origin, lower_left, horizontal, vertical)]
        _check(self._L.rt_hip_group_set_camera(self._h, *v), self._L)

    def set_lens(self, u, v, lens_radius):
        _check(self._L.rt_hip_group_set_lens(self._h, (C.c_double * 3)(*u), (C.c_double * 3)(*v), float(lens_radius)), self._L)

    def render_to_host(self, out=None):
        import numpy as np
        if out is None:
            out = np.zeros((self.height, self.width, 3), np.uint8)
        st = abi.RtStats()
        _check(self._L.rt_hip_group_render_to_host(self._h, out.ctypes.data, C.byref(st)), self._L)
        return out, st.as_dict()

    def render(self):
        """one frame, left in HBM of the group's first device (frame_ptr()); blocking; returns the stats"""
        st = abi.RtStats()
        _check(self._L.rt_hip_group_render(self._h, C.byref(st)), self._L)
        return st.as_dict()

    def submit(self, out=None):
        """enqueue one frame (rt_hip_group_submit); `out`: a numpy uint8 [h,w,3] array the frame is copied into (it must stay
        alive until the frame is collected), or None to leave it in HBM.  Two frames may be in flight."""
        _check(self._L.rt_hip_group_submit(self._h, out.ctypes.data if out is not None else None), self._L)

    def collect(self):
        """wait for the oldest submitted frame (rt_hip_group_collect); returns its stats"""
        st = abi.RtStats()
        _check(self._L.rt_hip_group_collect(self._h, C.byref(st)), self._L)
        return st.as_dict()

    def frame_ptr(self):
        """(device pointer of the assembled RGB8 frame collected last, device ordinal)"""
        dev = C.c_int(0)
        return self._L.rt_hip_group_frame(self._h, C.byref(dev)), dev.value

    def info(self):
        """what the group runs on: ranks, distinct devices, gather transport, RCCL communicators (rt_hip_group_info)"""
        gi = abi.RtGroupInfo()
        _check(self._L.rt_hip_group_info(self._h, C.byref(gi)), self._L)
        return {"n_ranks": gi.n_ranks, "n_devices": gi.n_devices, "transport": ("none", "rccl", "peer")[gi.transport],
                "rccl_comms": gi.rccl_comms, "tile_rows": gi.tile_rows, "pad_rows": gi.pad_rows, "emulated": bool(gi.emulated),
                "transport_fallback": bool(gi.transport_fallback),
                "fallback_reason": (self._L.rt_hip_group_fallback_reason(self._h) or b"").decode("utf-8", "replace"),
                "rank_devices": [gi.device[r] for r in range(min(gi.n_ranks, abi.RT_GROUP_INFO_MAX_RANKS))]}

    def ranks(self):
        """per rank: where it runs (device, PCI id, NUMA node, CPUs its host thread is pinned to, peer access to the first rank's
        device) and its share of the last frame (kernel_ms of the frame collected last; t_wake_us / t_enq_us of the frame submitted last)"""
        n = self._L.rt_hip_group_ranks(self._h, None, 0)
        arr = (abi.RtGroupRank * n)()
        self._L.rt_hip_group_ranks(self._h, arr, n)
        return [{"device": a.device, "pci_bus_id": a.pci_bus_id.decode("ascii", "replace"), "numa_node": a.numa_node, "pinned_cpus": a.pinned_cpus,
                 "peer_to_root": a.peer_to_root, "kernel_ms": a.kernel_ms, "t_wake_us": a.t_wake_us, "t_enq_us": a.t_enq_us} for a in arr]

    def close(self):
        if self._h:
            self._L.rt_hip_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_rgb8(scene_ptr):
    """rt_render_rgb8: host scene in, host RGB8 out (numpy [h,w,3]) + stats"""
    import numpy as np
    sc = scene_ptr.contents
    out = np.zeros((sc.height, sc.width, 3), np.uint8)
    st = abi.RtStats()
    _check(lib().rt_render_rgb8(scene_ptr, out.ctypes.data, C.byref(st)))
    return out, st.as_dict()
