"""tools/fuzz/fuzz_images.cpp — the host code of images on flat primitives (rt_flat_image.h, the loader, the writer) — built
with ASan + UBSan as a stand-alone program (its own main, no Python in the process) and run for a bounded number of iterations."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_images_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    exe = tmp_path / "fuzz_images"
    host = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "fuzz", "fuzz_images.cpp"), os.path.join(host, "scene.cpp"), os.path.join(host, "jpeg.cpp"),
                    "-I", os.path.join(ROOT, "include"), "-lz", "-lpthread", "-o", str(exe)], check=True)
    data = os.path.join(ROOT, "scenes", "data")
    for seed in (1, 2):
        r = subprocess.run([str(exe), str(seed), "12", os.path.join(data, "earth.jpg"), os.path.join(data, "beach.jpg")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-2000:])
        assert "round trips" in r.stdout and " 0 round trips" not in r.stdout and " 0 texels" not in r.stdout, r.stdout
        print(r.stdout.strip())
