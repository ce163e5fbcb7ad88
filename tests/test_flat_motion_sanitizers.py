"""tests/flatmotion/flat_motion_main.cpp — the host code of flat primitives that move within the frame (rt_flat_motion.h, the
swept boxes, the builder, the traversal beside the scan, the loader and the writer of "move") — built with ASan + UBSan as a stand-alone
program (its own main, no Python in the process) and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flat_motion_host_code_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    exe = tmp_path / "flat_motion_main"
    host = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DRT_TEST_PROBES", "-DRT_DEV_KNOBS", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "flatmotion", "flat_motion_main.cpp"), os.path.join(host, "scene.cpp"),
                    os.path.join(host, "jpeg.cpp"), "-I", os.path.join(ROOT, "include"), "-lz", "-lpthread", "-o", str(exe)], check=True)
    for seed in (1, 2):
        r = subprocess.run([str(exe), str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-2000:])
        assert "structure == scan" in r.stdout and "round trip of 11 entries" in r.stdout, r.stdout
        print(r.stdout.strip())
