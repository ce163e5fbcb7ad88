"""The prepare step of shading normals without a GPU: the device code of rt_flat_build.hip (flat_normals_prepare, what
rt_hip_scene_set_flat_normals runs for host and device input alike) compiled by g++ against the kernel-language emulation
(tests/flatupdate/emu), against the host build of rt_flat_normal_prepare: the table byte for byte, zero records flat, each refusal naming
the lowest bad k, parallelogram entries refused, the count of entries with normals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import smooth_mini as SMM
import smooth_points as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL = 0x7FF8DEADBEEF0000


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """as tests/test_flat_update_cpu.py builds it, behind the C interface of tests/smoothsim/flat_normals_emu.cpp"""
    hip_dir = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "hip")
    hdr = open(os.path.join(hip_dir, "rt_flat_build.h")).read()
    decl = hdr[hdr.index("#if defined(__HIPCC__)"):].replace("#if defined(__HIPCC__)", "").replace("#include <hip/hip_runtime.h>", "").rsplit("#endif", 1)[0]
    body = open(os.path.join(hip_dir, "rt_flat_build.hip")).read().replace("#include <hip/hip_runtime.h>", "").replace('#include "rt_flat_build.h"', "")
    d = tmp_path_factory.mktemp("flat_normals_emu")
    src = d / "emu.cpp"
    src.write_text('#include "hip/hip_runtime.h"\n#include "' + os.path.join(hip_dir, "rt_tables.h") + '"\n' + decl + body
                   + open(os.path.join(ROOT, "tests", "smoothsim", "flat_normals_emu.cpp")).read())
    so = d / "libflat_normals_emu.so"
    subprocess.run(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-DRT_TEST_PROBES", "-Wno-unknown-pragmas",
                    "-I", os.path.join(ROOT, "tests", "flatupdate", "emu"), str(src), "-o", str(so), "-lpthread"], check=True)
    L = C.CDLL(str(so))
    P, u32 = C.c_void_p, C.c_uint32
    L.fn_device.argtypes = [P, P, u32, P, P]
    L.fn_host.argtypes = [P, u32, P, P]
    L.fn_host.restype = None
    return L


def _device(emu, normals, lim):
    normals = np.ascontiguousarray(normals, np.float64)
    n = len(normals)
    out = np.full((n, 9), FILL, np.uint64)
    status = np.zeros(4, np.uint32)
    lim = None if lim is None else np.ascontiguousarray(lim, np.float64)
    assert emu.fn_device(normals.ctypes.data, None if lim is None else lim.ctypes.data, n, out.ctypes.data, status.ctypes.data) == 0
    return out, [int(x) for x in status]


def _host(emu, normals):
    normals = np.ascontiguousarray(normals, np.float64)
    out = np.full((len(normals), 9), FILL, np.uint64)
    kind = np.zeros(len(normals), np.int32)
    emu.fn_host(normals.ctypes.data, len(normals), out.ctypes.data, kind.ctypes.data)
    return out, kind


def _world(n=1000, seed=5):
    """n entries (several workgroups, the last one partial): every third without normals, every 50th a parallelogram without normals"""
    rng = np.random.default_rng(seed)
    normals = rng.uniform(-2, 2, (n, 9)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    normals[::3] = 0.0
    normals[6::9, 4] = -0.0
    lim = np.ones(n)
    lim[::150] = 2.0            # (multiples of 3: parallelograms, all without normals)
    return normals, lim


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_device_path_table_equals_the_host_path_table(emu):
    """a mixed list, and the generic, needle and scale tables of tests/smooth_points.py (the refused records of non_finite taken out):
    byte for byte the host's records, zero records flat, the count the number of entries with normals"""
    normals, lim = _world()
    got, status = _device(emu, normals, lim)
    want, kind = _host(emu, normals)
    assert (kind != SMM.BAD).all() and (kind[::3] == SMM.FLAT).all() and not want[::3].any()     # +0.0 and -0.0 alike: nine +0.0
    assert np.array_equal(got, want) and status == [NONE, NONE, int((kind == SMM.SMOOTH).sum()), 0]
    for cls in ("generic", "non_finite"):
        nr = SP.table(cls)[1][:30_000]
        want, kind = _host(emu, nr)
        ok = kind != SMM.BAD
        got, status = _device(emu, nr[ok], np.ones(int(ok.sum())))
        assert np.array_equal(got, want[ok]) and status == [NONE, NONE, int((kind == SMM.SMOOTH).sum()), 0], cls
        for i in np.flatnonzero(ok)[:2000]:
            k, r = SMM.prepare(nr[i])
            assert k == kind[i] and np.array_equal(np.array(r).view(np.uint64), want[i]), (cls, i)


def test_each_refusal_names_the_lowest_bad_entry(emu):
    normals, lim = _world()
    for bad_at, what in (([700, 40, 301], "nan"), ([999], "inf"), ([64, 65], "zero vector"), ([513], "tiny"), ([257, 255], "huge")):
        nr = normals.copy()
        for k in bad_at:
            nr[k] = [0.3, 0.2, 1.0, 0.1, 1.0, 0.0, 1.0, 0.0, 0.2]
            if what == "nan":
                nr[k, 4] = np.nan
            elif what == "inf":
                nr[k, 8] = -np.inf
            elif what == "zero vector":
                nr[k, 3:6] = 0.0
            elif what == "tiny":
                nr[k, 0:3] = [1e-170, 0.0, 0.0]
            else:
                nr[k, 6:9] = [1e160, 0.0, 0.0]
        got, status = _device(emu, nr, lim)
        assert status[0] == min(bad_at) and status[1] == NONE, (what, status)
        assert (got[bad_at] == FILL).all()                                    # a refused entry writes nothing
        assert _host(emu, nr)[1][bad_at].tolist() == [SMM.BAD] * len(bad_at)


def test_parallelogram_entries_are_refused(emu):
    normals, lim = _world()
    nr = normals.copy()
    nr[450] = nr[300] = [0, 0, 1.0, 0, 0, 1.0, 0, 0, 1.0]                    # two parallelograms with normals
    _, status = _device(emu, nr, lim)
    assert status[:2] == [NONE, 300]
    nr[20, 0] = np.nan                                                        # ... and a refused vector below them: both classes, each its lowest
    _, status = _device(emu, nr, lim)
    assert status[:2] == [20, 300]
    tri_only = normals.copy(); tri_only[::3] = [0, 0, 1.0, 0, 0, 1.0, 0, 0, 1.0]
    _, status = _device(emu, tri_only, None)                                  # a scene without a limit table: every entry a parallelogram
    assert status[:2] == [NONE, 0]
    got, status = _device(emu, np.zeros((70, 9)), None)                       # ... which may still say "none" for every entry
    assert status == [NONE, NONE, 0, 0] and not got.any()
