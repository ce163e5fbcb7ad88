#!/usr/bin/env python3
"""Correctly rounded -ln(x) of the arguments below, by mpmath at 200 bits (the double nearest the true value; a result within 2^-140 of a
rounding boundary would need more, none is).  Writes tests/golden/neg_log_cr.npz: the argument bits (u64), the correctly rounded result
(f64), the part of the true value the rounding took away in ulps of the result (f32, so that an error can be measured against the true
value to 2^-24 ulp) and the categories as "name:count", in argument order.  tests/test_medium_cpu.py holds csrc/common/rt_neg_log.h to its own claim with
it: an error below 1 ulp of the correctly rounded value.

The arguments (a medium draws x = 1 - u, u = k 2^-53, so 1 - k 2^-53 is what the kernel evaluates; the rest are the routine's own edges):
  random     1 - k 2^-53, k random over every magnitude
  smallest   the 5 000 smallest k (x just below 1: f tiny, the result is all cancellation)
  largest    the 5 000 largest k (x = j 2^-53: the exponent term dominates)
  sqrt2      in each binade 2^-53 .. 2^-1 the five mantissas 0x6A09E667F3BCD + {-2 .. 2}: either side of the switch of step 2
  pow2       every power of two, 2^-1074 .. 2^1023 (the subnormal ones included; 1.0 is asserted apart and left out)
  subnormal  ten subnormals with full mantissas
The file is written with fixed zip time stamps, so that a second run gives the same bytes:

    python tests/golden/make_neg_log_fixture.py            (~10 s; --check compares with the committed file instead of writing)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "neg_log_cr.npz")
SQRT2_MANT = 0x6A09E667F3BCD


def arguments():
    """-> x (f64, every one finite and > 0, none 1.0), [(category, count)] in order"""
    rng = np.random.default_rng(1515)
    one_minus = lambda k: 1.0 - k.astype(np.float64) * 2.0 ** -53      # (exact: k < 2^53)
    k_rand = np.concatenate([rng.integers(1, 1 << 53, 6_000, dtype=np.uint64),
                             (rng.integers(1, 1 << 53, 9_000, dtype=np.uint64) >> rng.integers(0, 52, 9_000).astype(np.uint64)) | np.uint64(1)])
    sqrt2 = np.array([((1023 - b) << 52) | (SQRT2_MANT + d) for b in range(1, 54) for d in range(-2, 3)], np.uint64).view(np.float64)
    pow2 = np.array([2.0 ** e for e in range(-1074, 1024) if e != 0])
    sub = rng.integers(1, 1 << 52, 10, dtype=np.uint64).view(np.float64)
    parts = [("random", one_minus(k_rand)), ("smallest", one_minus(np.arange(1, 5_001, dtype=np.uint64))),
             ("largest", one_minus(np.uint64((1 << 53) - 1) - np.arange(0, 5_000, dtype=np.uint64))), ("sqrt2", sqrt2), ("pow2", pow2), ("subnormal", sub)]
    x = np.concatenate([p for _, p in parts])
    assert len(x) <= 60_000 and (x > 0.0).all() and np.isfinite(x).all() and (x != 1.0).all()
    return x, [(n, len(p)) for n, p in parts]


def correctly_rounded(x):
    """-> the correctly rounded -ln x (f64), and what rounding it took away: (true value - rounded) / ulp(rounded) as f32, in [-1/2, 1/2]"""
    import mpmath as mp
    mp.mp.prec = 200
    cr, res = np.empty(len(x)), np.empty(len(x), np.float32)
    for i, v in enumerate(x.tolist()):
        true = -mp.log(mp.mpf(v))
        cr[i] = float(true)                                               # mpf -> float rounds to nearest even
        res[i] = float((true - mp.mpf(float(cr[i]))) / mp.mpf(float(np.spacing(abs(cr[i])))))
    return cr, res


def fixture_bytes():
    x, cats = arguments()
    cr, res = correctly_rounded(x)
    arrays = {"x_bits": x.view(np.uint64), "neg_log": cr, "residual_ulp": res, "categories": np.array([f"{n}:{c}" for n, c in cats])}
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    return out.getvalue(), cats


def main():
    data, cats = fixture_bytes()
    if "--check" in sys.argv:
        same = open(PATH, "rb").read() == data
        print("the committed fixture is", "reproduced byte for byte" if same else "NOT what this generator writes")
        return 0 if same else 1
    open(PATH, "wb").write(data)
    print(len(data), "bytes", cats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
