"""Regenerates tests/golden/narrow/*.npz from the REAL reference: tests/golden/narrow/narrow_driver.cpp (this repository's text) is compiled in
a scratch directory against the reference's headers and a config.hh made by oracle/gen_config.cmake, and run once per case.

    python tests/golden/narrow/make_golden_narrow.py REFERENCE_ROOT

Every file holds: kind (the library's FTKX_DTYPE_* code of the source's element type), dims (x first), input (numpy C order with x last, in
its own element type), out_shape (the reference's shape of the result, first index fastest) and output (float64, flat):
ndarray<double>::from_array(ndarray<T1>(input)).  The integer inputs carry 0, +-1 and the type's extremes among seeded values; float32 is
there as the control (the conversion tests/golden/concat/ already holds numpy to).  The reference has no half or bfloat16 type.
No test runs this script or reads the reference."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))

SHAPES = ((5, 3), (3, 2, 2))          # x first
KINDS = {1: ("f32", np.float32), 4: ("u8", np.uint8), 5: ("i8", np.int8), 6: ("u16", np.uint16), 7: ("i16", np.int16), 8: ("u32", np.uint32), 9: ("i32", np.int32)}


def input_of(dtype, dims, seed):
    rng = np.random.default_rng(seed)
    shape = tuple(reversed(dims))
    if dtype == np.float32:
        a = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
        special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x007fffff, 0x7f7fffff], dtype=np.uint32).view(np.float32)
    else:
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max, size=shape, dtype=np.int64, endpoint=True).astype(dtype)
        special = np.array([v for v in (0, 1, -1, info.min, info.max, info.max // 2 + 1) if info.min <= v <= info.max], dtype=np.int64).astype(dtype)
    at = rng.permutation(a.size)[:len(special)]
    a.reshape(-1)[at] = special
    return a


def build_driver(ref, work):
    subprocess.check_call(["cmake", "-DREF=" + ref, "-DOUT=" + work, "-P", os.path.join(ROOT, "oracle", "gen_config.cmake")])
    exe = os.path.join(work, "narrow_driver")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-w", "-I" + os.path.join(ref, "include"), "-I" + os.path.join(work, "include"), "-o", exe,
                           os.path.join(HERE, "narrow_driver.cpp"), "-lpthread"])
    return exe


def reference_from_array(exe, work, kind, a, dims):
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        np.array([kind, len(dims)] + list(dims), dtype=np.int64).tofile(f)
        np.ascontiguousarray(a).tofile(f)
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        nd = int(np.fromfile(f, dtype=np.int64, count=1)[0])
        shape = np.fromfile(f, dtype=np.int64, count=nd)
        out = np.fromfile(f, dtype=np.float64, count=int(np.prod(shape)))
    assert out.size == a.size, (shape, a.shape)
    return shape, out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    with tempfile.TemporaryDirectory() as work:
        exe = build_driver(ref, work)
        seed = 70
        for kind, (name, dtype) in sorted(KINDS.items()):
            for dims in SHAPES:
                seed += 1
                a = input_of(dtype, dims, seed)
                shape, out = reference_from_array(exe, work, kind, a, dims)
                np.savez_compressed(os.path.join(HERE, "narrow_%s_%s.npz" % (name, "x".join(str(d) for d in dims))), kind=kind, dims=np.array(dims), input=a, out_shape=shape,
                                    output=out)


if __name__ == "__main__":
    main()
