"""Spatial Gaussian smoothing as the library and the package offer it; nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import conv_cases as CC

NEW = ["ftkx_gaussian_kernel", "ftkx_conv2D", "ftkx_conv3D", "ftkx_set_spatial_smoothing", "ftkx_tracker_set_spatial_smoothing"]


@pytest.fixture(scope="module")
def L():
    from ftk_amd import _lib, build
    build.build()
    return _lib.load()


def test_library_exports_the_new_functions(L):
    from ftk_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(raw, name) is not None
        assert getattr(L, name).argtypes is not None, name
    import ftk_amd
    for m in ("set_spatial_smoothing", "conv2D", "conv3D"):
        assert hasattr(ftk_amd.Context, m)
    assert hasattr(ftk_amd.CriticalPointTracker2DRegular, "set_spatial_smoothing") and "gaussian_kernel" in ftk_amd.__all__


@pytest.mark.parametrize("name", CC.fixture_names() + ["series_woven_noisy_31x37x8_k3"])
def test_gaussian_kernel_is_the_references(L, name):
    """(the fixtures' weights come from the C library's exp of the machine that wrote them: this holds where that exp agrees)"""
    import ftk_amd
    f = CC.load(name)
    w = ftk_amd.gaussian_kernel(int(f["nd"]), float(f["sigma"]), int(f["ksize"]))
    assert w.shape == f["weights"].shape
    assert np.array_equal(w.view(np.uint64), f["weights"].view(np.uint64))


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_gaussian_kernel_every_size(L, nd, ksize):
    import ftk_amd
    for sigma in (0.5, 1.0, 2.75):
        assert np.array_equal(ftk_amd.gaussian_kernel(nd, sigma, ksize).view(np.uint64), CC.gaussian_weights(nd, sigma, ksize).view(np.uint64))


def test_argument_errors_without_a_gpu(L):
    from ftk_amd import _lib
    import ftk_amd
    w = np.zeros(729)
    for nd, sigma, ksize in [(1, 1.0, 3), (4, 1.0, 3), (2, 1.0, 4), (3, 1.0, 2), (2, 1.0, 0), (2, 1.0, -3), (3, 1.0, 11), (2, 0.0, 3), (2, -1.0, 3),
                             (2, float("nan"), 3), (3, float("inf"), 5)]:
        assert L.ftkx_gaussian_kernel(nd, sigma, ksize, w.ctypes.data) == _lib.E_INVALID, (nd, sigma, ksize)
        with pytest.raises(ftk_amd.FtkxError):
            ftk_amd.gaussian_kernel(nd, sigma, ksize)
    assert L.ftkx_gaussian_kernel(2, 1.0, 3, None) == _lib.E_INVALID
    assert not w.any()
    assert L.ftkx_set_spatial_smoothing(None, 1.0, 3) == _lib.E_INVALID
    assert L.ftkx_set_spatial_smoothing(None, 0.0, 0) == _lib.E_INVALID
    assert L.ftkx_conv2D(None, None, 4, 4, w.ctypes.data, 3, None) == _lib.E_INVALID
    assert L.ftkx_conv3D(None, None, 4, 4, 4, w.ctypes.data, 3, None) == _lib.E_INVALID
    assert L.ftkx_tracker_set_spatial_smoothing(None, 1.0, 3) == _lib.E_INVALID
    buf = C.create_string_buffer(256)
    L.ftkx_gaussian_kernel(2, 1.0, 4, w.ctypes.data)
    L.ftkx_last_error(None, buf, 256)
    assert b"ksize" in buf.value
