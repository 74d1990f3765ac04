"""The oracle of the planar GPU tests against the REAL reference, without a GPU: tests/golden/concat/*.npz hold what ndarray<T>::concat (and,
for float32 planes, ndarray<double>::from_array behind it) made of a few tiny inputs -- nc 2 and 3, 5 x 3 and 3 x 2 x 2, with zeros of either
sign, infinities, subnormals and quiet NaNs of both signs among the values (tests/golden/concat/make_golden_concat.py).  The numpy
expression that tests/test_gpu_planar.py and tests/test_concat_host.py hold the kernel to is held to these files bit for bit here."""
import glob
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(HERE, "golden", "concat", "concat_*.npz")))


def interleave(planes):
    """THE oracle: components fastest, then widened"""
    return np.stack(list(planes), axis=-1).reshape(-1).astype(np.float64)


def test_fixtures_are_all_there():
    names = {os.path.basename(f) for f in FILES}
    assert names == {"concat_%s_nc%d_%s.npz" % (t, nc, s) for t in ("f32", "f64") for nc in (2, 3) for s in ("5x3", "3x2x2")}, names


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_numpy_interleave_is_the_references_concat(path):
    g = np.load(path)
    planes, out, nc, dims = g["planes"], g["output"], int(g["nc"]), [int(d) for d in g["dims"]]
    assert planes.shape == (nc,) + tuple(reversed(dims)) and planes.dtype in (np.float32, np.float64) and out.dtype == np.float64
    assert [int(d) for d in g["out_shape"]] == [nc] + dims                     # the components are the reference's first (fastest) index
    # the inputs are what the issue of this feature asks for: every class of value is among them
    flat = planes.reshape(-1)
    tiny = np.finfo(planes.dtype).tiny
    assert np.any((flat == 0) & np.signbit(flat)) and np.any((flat == 0) & ~np.signbit(flat))
    assert np.any(np.isposinf(flat)) and np.any(np.isneginf(flat))
    assert np.any(np.isnan(flat) & np.signbit(flat)) and np.any(np.isnan(flat) & ~np.signbit(flat))
    with np.errstate(invalid="ignore"):
        assert np.any((np.abs(flat) < tiny) & (flat != 0))
    got = interleave(planes)
    assert got.shape == out.shape
    nan = np.isnan(out)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.signbit(got), np.signbit(out))
    assert np.array_equal(got.view(np.uint64)[~nan], out.view(np.uint64)[~nan])
    if planes.dtype == np.float64:          # FP64 is moved, payloads and all
        assert np.array_equal(got.view(np.uint64), out.view(np.uint64))
    # ... and the separate-tensor and the (nc, ...) forms of the planes are one thing
    assert np.array_equal(interleave([planes[k] for k in range(nc)]).view(np.uint64), got.view(np.uint64))
