"""In-tree build of the native pieces (no cmake; plain g++ / hipcc command lines)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra"]
# RT_WAVES_PER_EU=4: cap the megakernel at 128 VGPRs (4 waves/SIMD); measured best of 2/3/4/5 (profiles/r01_run2_ab.log)
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRT_WAVES_PER_EU=4"]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd):
    print("+", " ".join(cmd), file=sys.stderr, flush=True)
    subprocess.run(cmd, check=True, cwd=HERE)


def _srcs(*rel):
    return [os.path.join(HERE, r) for r in rel]


def build_host(force=False):
    out = os.path.join(HERE, "librt_host.so")
    src = _srcs("csrc/host/scene.cpp", "csrc/host/jpeg.cpp")
    deps = src + _srcs("csrc/host/json.hpp", "csrc/common/rt_quad.h", "csrc/common/rt_flat_light.h", "csrc/common/rt_flat_normal.h",
                      "csrc/common/rt_flat_image.h") + [os.path.join(ROOT, "include/rt_abi.h")]
    if force or _newer(out, deps):
        _run(["g++", *CXXFLAGS, "-shared", *src, "-o", out, "-lz", "-lpthread"])
    return out


def build_hip(force=False):
    """librt_hip.so = the product (include/rt_abi.h, nothing else exported); librt_hip_probe.so = the same sources with
    -DRT_TEST_PROBES: + the device probes and debug calls of include/rt_abi_test.h, for tests/ and tools/diag.py only"""
    out = os.path.join(HERE, "librt_hip.so")
    probe = os.path.join(HERE, "librt_hip_probe.so")
    deps = _srcs(*HIP_DEPS) + [os.path.join(ROOT, "include/rt_abi.h"), os.path.join(ROOT, "include/rt_abi_test.h"),
                                 os.path.join(ROOT, "include/rt_abi_test_flat_light.h"), os.path.join(ROOT, "include/rt_abi_test_flat_image.h"),
                                 os.path.join(ROOT, "include/rt_abi_test_flat_motion.h")]
    # (beside the file times: the source hash the libraries on disk were built from — a checkout or a clock that does not move
    #  forward leaves times that say nothing)
    try:
        import json
        built_from = json.load(open(os.path.join(HERE, "BUILD_INFO.json"))).get("kernel_src_hash")
    except Exception:
        built_from = None
    if os.path.exists(os.path.join(ROOT, ".git")) and built_from != kernel_src_hash():
        force = True
    # (linked against librt_host.so: rt_abi.h is one seam, and a handle of librt_hip.so resolves its host calls — the scene file
    #  and camera helpers — too)
    link = ["-L" + HERE, "-Wl,--no-as-needed", "-lrt_host", "-Wl,-rpath,$ORIGIN"]
    # HIP_UNITS per library, compiled side by side, each about a minute of one core (one unit with the megakernel's 288 instantiations
    # was many times that).  Objects under build/ (git-ignored), then one link per library.
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    compiles, links = [], []
    for lib, extra in ((out, []), (probe, ["-DRT_TEST_PROBES"])):
        if not (force or _newer(lib, deps)):
            continue
        objs = []
        for name, unit, defs in HIP_UNITS:
            obj = os.path.join(objdir, name + ("_probe" if extra else "") + ".o")
            compiles.append(["hipcc", *HIPFLAGS, *extra, *defs, "-c", os.path.join(HERE, unit), "-o", obj])
            objs.append(obj)
        links.append(["hipcc", *HIPFLAGS, "-shared", *objs, "-o", lib, *link])
    for batch in (compiles, links):
        procs = []
        for cmd in batch:   # (side by side)
            print("+", " ".join(cmd), file=sys.stderr, flush=True)
            procs.append((cmd, subprocess.Popen(cmd, cwd=HERE)))
        for cmd, pr in procs:
            if pr.wait() != 0:
                raise subprocess.CalledProcessError(pr.returncode, cmd)
    return out


def build_cli(force=False):
    """the `raytracer <config_file> <output_file>` binary (reference main.rs)"""
    out = os.path.join(HERE, "raytracer")
    src = _srcs("csrc/host/main.cpp")
    deps = src + _srcs("csrc/host/anim_path.h", "csrc/host/cli_args.h") + [os.path.join(HERE, "librt_host.so"), os.path.join(HERE, "librt_hip.so")]
    if os.path.exists(src[0]) and (force or _newer(out, deps)):
        _run(["g++", *CXXFLAGS, *src, "-o", out, "-L" + HERE, "-lrt_host", "-lrt_hip", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    return out


# The translation units of librt_hip.so as (object name, source, defines): rt_hip_api.hip with kernel set 0 (the megakernel instantiations
# with key >> 6 == 0, csrc/hip/rt_kernel.hip) and everything else; rt_kernel_set.hip once for each of the sets 1 - 15 (MOTION, DESIGN.md §14;
# MEDIUM, §15; SOLID, §16; QUADS, §20: the sets 8 - 15, eight kernels each); the device grid build of rt_hip_scene_update_spheres (§17: a few
# small kernels); the records and the refit of rt_hip_scene_update_flats (§24: three small kernels) and the order
# table built on the device (§26: four small kernels and rocprim's merge sort).
HIP_UNITS = ([("rt_hip_api", "csrc/hip/rt_hip_api.hip", ["-DRT_KERNEL_SET_SPLIT"])]
             + [("rt_kernel_set%d" % k, "csrc/hip/rt_kernel_set.hip", ["-DRT_KERNEL_SET=%d" % k]) for k in range(1, 16)]
             + [("rt_grid_build", "csrc/hip/rt_grid_build.hip", []), ("rt_flat_build", "csrc/hip/rt_flat_build.hip", [])])
# what the units are compiled from: every unit, and the files they include
HIP_DEPS = tuple(dict.fromkeys(u for _, u, _ in HIP_UNITS)) + (
    "csrc/hip/rt_kernel.hip", "csrc/hip/rt_hip_flats.hip", "csrc/hip/rt_hip_group.hip", "csrc/hip/rt_core.h", "csrc/hip/rt_tables.h", "csrc/hip/rt_grid_build.h",
    "csrc/hip/rt_flat_build.h",
    "csrc/common/rt_atan2.h", "csrc/common/rt_neg_log.h", "csrc/common/rt_solid.h", "csrc/common/rt_quad.h",
    "csrc/common/rt_flat_normal.h", "csrc/common/rt_flat_motion.h", "csrc/common/rt_flat_light.h", "csrc/common/rt_flat_image.h")


def kernel_src_hash():
    """sha1 over the sources librt_hip.so is compiled from: what a counter file and a bench run must share to describe the
    same kernel (a commit id changes with every documentation commit; this does not)"""
    import hashlib
    h = hashlib.sha1()
    for f in _srcs(*HIP_DEPS) + [os.path.join(ROOT, "include/rt_abi.h")]:
        h.update(open(f, "rb").read())
    h.update((" ".join(HIPFLAGS) + repr(HIP_UNITS)).encode())
    return h.hexdigest()[:12]


def write_build_info():
    """BUILD_INFO.json next to the libraries: the commit they were built from.  The GPU box gets a snapshot without .git,
    so bench.py and the PMC tools read the head from here (git-ignored, travels with the .so files)."""
    import json
    import time

    def git(*a):
        try:
            return subprocess.run(["git", *a], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip()
        except Exception:
            return ""
    head = git("rev-parse", "--short", "HEAD")
    if not head:
        return  # (not a git checkout: keep whatever file travelled with the snapshot)
    dirty = bool(git("status", "--porcelain", "--untracked-files=no"))
    info = {"git_head": head + ("+dirty" if dirty else ""), "built_at": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
            "kernel_src_hash": kernel_src_hash()}
    with open(os.path.join(HERE, "BUILD_INFO.json"), "w") as f:
        json.dump(info, f)


def build_all(force=False):
    build_host(force)
    build_hip(force)
    build_cli(force)
    write_build_info()


if __name__ == "__main__":
    build_all("--force" in sys.argv)
