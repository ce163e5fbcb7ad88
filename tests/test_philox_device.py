"""The megakernel's Philox4x32-10 as the GPU runs it (rt_core.h: each round's three-input XOR is one v_bitop3_b32 on
gfx950), against the Random123 known answers and the pure-Python Philox of tests/mini_oracle.py: a standalone program
(tests/philox_device.hip) built with the product's flags runs both device forms of the call."""
import os
import subprocess

import numpy as np
import pytest

import mini_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRT_WAVES_PER_EU=4"]  # build.py's
NODE_CAMERA = 0xFFFFFFFF
PI = [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]
KAT = [([0] * 4, [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       (PI, [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


def philox_np(ctr, key):
    """mini_oracle.philox4x32_10 on arrays (uint64 holds every 32 x 32-bit product)"""
    c = [ctr[:, j].astype(np.uint64) for j in range(4)]
    k0, k1 = key[:, 0].astype(np.uint64), key[:, 1].astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


def cases(n_waves=16384, seed=20261015):
    """n_waves x 64 counters; one key per wave (the device's rng() form needs a wave-uniform key).  Wave w < 3 opens with
    known answer w; a quarter of the waves are camera draws (node NODE_CAMERA, slot 0), a quarter run slots 0 .. 63 or 1 .. 64
    of one (pixel, sample, node), the rest are random counters."""
    rng = np.random.default_rng(seed)
    n = 64 * n_waves
    ctr = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    wkey = rng.integers(0, 1 << 32, size=(n_waves, 2), dtype=np.uint64).astype(np.uint32)
    for w, (c, k, _) in enumerate(KAT):
        ctr[64 * w] = c
        wkey[w] = k
    cam = np.arange(4, n_waves, 4)
    rows = (64 * cam[:, None] + np.arange(64)).ravel()
    ctr[rows, 2], ctr[rows, 3] = NODE_CAMERA, 0
    slots = np.arange(5, n_waves, 4)
    rows = 64 * slots[:, None] + np.arange(64)
    ctr[rows, 3] = np.arange(64, dtype=np.uint32) + ((slots // 4) % 2).astype(np.uint32)[:, None]  # slots 0 .. 63 or 1 .. 64
    for j in range(3):
        ctr[rows, j] = ctr[rows[:, :1], j]
    return ctr, np.repeat(wkey, 64, axis=0)


def test_numpy_philox_is_the_mini_oracle():
    ctr, key = cases(n_waves=16)
    got = philox_np(ctr, key)
    for i in range(len(ctr)):
        assert tuple(int(x) for x in got[i]) == mini_oracle.philox4x32_10(*(int(x) for x in ctr[i]), *(int(x) for x in key[i]))
    for w, (_, _, want) in enumerate(KAT):
        assert list(got[64 * w]) == want


@pytest.mark.gpu
def test_device_philox_matches_random123_and_the_oracle(tmp_path):
    exe = str(tmp_path / "philox_device")
    subprocess.run(["hipcc", *HIPFLAGS, os.path.join(ROOT, "tests", "philox_device.hip"), "-o", exe], check=True, timeout=600)
    ctr, key = cases()
    n = len(ctr)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.uint32(n).tobytes() + ctr.tobytes() + key.tobytes())
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=120)
    out = np.fromfile(outp, dtype=np.uint32).reshape(2, n, 4)
    want = philox_np(ctr, key)
    for w, (_, _, kat) in enumerate(KAT):
        assert list(out[0, 64 * w]) == kat and list(out[1, 64 * w]) == kat
    for form in range(2):
        bad = np.flatnonzero((out[form] != want).any(axis=1))
        assert bad.size == 0, (form, bad[:8], ctr[bad[:8]], key[bad[:8]])
