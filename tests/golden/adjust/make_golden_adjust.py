"""Regenerates tests/golden/adjust/clamp.npz from the REAL reference: tests/golden/adjust/clamp_driver.cpp (this repository's text) is compiled
in a scratch directory against the reference's headers and a config.hh made by oracle/gen_config.cmake, and run once per pair of bounds.

    python tests/golden/adjust/make_golden_adjust.py REFERENCE_ROOT

The file holds, as uint64 bit patterns (NaN signs and payloads survive): values (n), bounds (5 pairs lo, hi), outputs (5 x n) =
ndarray<double>::clamp(lo, hi) of the values.  No test runs this script or reads the reference."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))

BOUNDS = [(-1.0, 1.0), (0.0, 0.0), (-0.0, 0.0), (1.0, -1.0), (-np.inf, 5.0)]


def values():
    """+-0, +-inf, +-NaN, subnormals, +-DBL_MAX; every bound and one ulp either side of it; random bit patterns up to 64 values"""
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308,
         np.finfo(np.float64).max, -np.finfo(np.float64).max]
    for b in (-1.0, 1.0, 5.0):
        v += [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
    a = np.array(v, dtype=np.float64).view(np.uint64)
    a[5] |= np.uint64(1) << np.uint64(63)          # (-np.nan may or may not carry the sign: set it)
    extra = np.array([0x7ff8000000000123, 0xfff4000000000001], dtype=np.uint64)      # a quiet NaN with a payload, a negative signalling one
    rnd = np.random.default_rng(20).integers(0, 2 ** 64, size=64 - len(a) - len(extra), dtype=np.uint64)
    return np.concatenate([a, extra, rnd])


def build_driver(ref, work):
    subprocess.check_call(["cmake", "-DREF=" + ref, "-DOUT=" + work, "-P", os.path.join(ROOT, "oracle", "gen_config.cmake")])
    exe = os.path.join(work, "clamp_driver")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-w", "-I" + os.path.join(ref, "include"), "-I" + os.path.join(work, "include"), "-o", exe,
                           os.path.join(HERE, "clamp_driver.cpp"), "-lpthread"])
    return exe


def reference_clamp(exe, work, bits, lo, hi):
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qdd", len(bits), lo, hi))
        bits.tofile(f)
    subprocess.check_call([exe, src, dst])
    return np.fromfile(dst, dtype=np.uint64, count=len(bits))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    v = values()
    with tempfile.TemporaryDirectory() as work:
        exe = build_driver(ref, work)
        out = np.stack([reference_clamp(exe, work, v, lo, hi) for lo, hi in BOUNDS])
    np.savez_compressed(os.path.join(HERE, "clamp.npz"), values=v, bounds=np.array(BOUNDS, dtype=np.float64).view(np.uint64), outputs=out)


if __name__ == "__main__":
    main()
