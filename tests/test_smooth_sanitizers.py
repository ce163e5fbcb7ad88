"""tools/fuzz/fuzz_normals.cpp — the host code of shading normals (rt_flat_normal.h, the loader, the writer) — built with
ASan + UBSan as a stand-alone program (its own main, no Python in the process) and run for a bounded number of iterations."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_normals_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    exe = tmp_path / "fuzz_normals"
    host = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "fuzz", "fuzz_normals.cpp"), os.path.join(host, "scene.cpp"), os.path.join(host, "jpeg.cpp"),
                    "-I", os.path.join(ROOT, "include"), "-lz", "-lpthread", "-o", str(exe)], check=True)
    for seed in (1, 2):
        r = subprocess.run([str(exe), str(seed), "60"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-2000:])
        assert "round trips" in r.stdout, r.stdout
        print(r.stdout.strip())
