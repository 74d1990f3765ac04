"""Regenerates tests/golden/concat/*.npz from the REAL reference: tests/golden/concat/concat_driver.cpp (this repository's text) is compiled in
a scratch directory against the reference's headers and a config.hh made by oracle/gen_config.cmake, and run once per case.

    python tests/golden/concat/make_golden_concat.py REFERENCE_ROOT

Every file holds: nc, dims (x first), planes (nc arrays in numpy C order with x last, float32 or float64), out_shape (the reference's shape
of the result, first index fastest) and output (float64, flat): ndarray<T>::concat(planes), widened with ndarray<double>::from_array where
the planes are float32.  The planes carry zeros of either sign, infinities, subnormals and quiet NaNs of both signs among seeded values.
No test runs this script or reads the reference."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))

SHAPES = ((5, 3), (3, 2, 2))          # x first
SPECIAL32 = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x7fc00000, 0xffc00000, 0x7fc12345, 0xffc54321], dtype=np.uint32)
SPECIAL64 = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x7ff8000000000000,
                      0xfff8000000000000, 0x7ff8000000abcdef, 0xfffc0000deadbeef], dtype=np.uint64)


def planes_of(dtype, nc, dims, seed):
    """nc seeded planes in [-1, 1) with the special values strewn over them (every one of them lands somewhere)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=(nc,) + tuple(reversed(dims))).astype(dtype)
    special = (SPECIAL32 if dtype == np.float32 else SPECIAL64).view(dtype)
    at = rng.permutation(a.size)[:len(special)]
    a.reshape(-1)[at] = special
    return a


def build_driver(ref, work):
    subprocess.check_call(["cmake", "-DREF=" + ref, "-DOUT=" + work, "-P", os.path.join(ROOT, "oracle", "gen_config.cmake")])
    exe = os.path.join(work, "concat_driver")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-w", "-I" + os.path.join(ref, "include"), "-I" + os.path.join(work, "include"), "-o", exe,
                           os.path.join(HERE, "concat_driver.cpp"), "-lpthread"])
    return exe


def reference_concat(exe, work, planes, dims):
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        np.array([int(planes.dtype == np.float32), planes.shape[0], len(dims)] + list(dims), dtype=np.int64).tofile(f)
        np.ascontiguousarray(planes).tofile(f)
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        nd = int(np.fromfile(f, dtype=np.int64, count=1)[0])
        shape = np.fromfile(f, dtype=np.int64, count=nd)
        out = np.fromfile(f, dtype=np.float64, count=int(np.prod(shape)))
    assert out.size == planes.size, (shape, planes.shape)
    return shape, out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    with tempfile.TemporaryDirectory() as work:
        exe = build_driver(ref, work)
        seed = 40
        for dtype in (np.float32, np.float64):
            for nc in (2, 3):
                for dims in SHAPES:
                    seed += 1
                    planes = planes_of(dtype, nc, dims, seed)
                    shape, out = reference_concat(exe, work, planes, dims)
                    name = "concat_%s_nc%d_%s" % ("f32" if dtype == np.float32 else "f64", nc, "x".join(str(d) for d in dims))
                    np.savez_compressed(os.path.join(HERE, name + ".npz"), nc=nc, dims=np.array(dims), planes=planes, out_shape=shape, output=out)


if __name__ == "__main__":
    main()
