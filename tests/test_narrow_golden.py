"""The yardstick of the narrow-type tests against the REAL reference, without a GPU: tests/golden/narrow/*.npz hold what
ndarray<double>::from_array(ndarray<T1>) made of a few tiny inputs -- unsigned char, signed char, unsigned short, short, unsigned int, int,
and float as the control; 5 x 3 and 3 x 2 x 2; 0, +-1 and the type's extremes among the values (tests/golden/narrow/make_golden_narrow.py).
numpy's astype(float64), which tests/test_narrow_host.py and tests/test_gpu_narrow.py hold the kernel to, is held to these files bit for bit
here."""
import glob
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(HERE, "golden", "narrow", "narrow_*.npz")))
KINDS = {"f32": (1, np.float32), "u8": (4, np.uint8), "i8": (5, np.int8), "u16": (6, np.uint16), "i16": (7, np.int16), "u32": (8, np.uint32), "i32": (9, np.int32)}


def test_fixtures_are_all_there():
    names = {os.path.basename(f) for f in FILES}
    assert names == {"narrow_%s_%s.npz" % (t, s) for t in KINDS for s in ("5x3", "3x2x2")}, names


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_numpy_astype_is_the_references_from_array(path):
    g = np.load(path)
    a, out, kind, dims = g["input"], g["output"], int(g["kind"]), [int(d) for d in g["dims"]]
    code, dtype = KINDS[os.path.basename(path).split("_")[1]]
    assert kind == code and a.dtype == dtype and a.shape == tuple(reversed(dims)) and out.dtype == np.float64
    assert [int(d) for d in g["out_shape"]] == dims                     # from_array keeps the shape
    flat = a.reshape(-1)
    if a.dtype.kind in "iu":          # the values at which a conversion can go wrong are among the inputs
        info = np.iinfo(a.dtype)
        for v in (0, 1, info.min, info.max, info.max // 2 + 1) + ((-1,) if info.min < 0 else ()):
            assert np.any(flat == v), (a.dtype, v)
    got = flat.astype(np.float64)
    assert got.shape == out.shape and np.array_equal(got.view(np.uint64), out.view(np.uint64))
    assert np.array_equal(out.astype(a.dtype), flat)                    # ... and exact: it converts back
