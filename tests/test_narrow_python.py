"""The Python layer's handling of narrow element types WITHOUT a GPU (ftk_amd/__init__.py: _ptr_typed, _one_dtype, _TrackerRegular._narrow):
which element types are taken, that nothing is copied for a contiguous array, and that the contiguous copy made of a view that is not
contiguous is handed to the caller together with its address -- the library reads that copy, so it has to live until the call returns."""
import numpy as np
import pytest

import ftk_amd


class Holder:
    """what _narrow needs of a tracker"""
    def __init__(self):
        self._keep = []


def test_contiguous_arrays_are_taken_as_they_are():
    for dtype, code in ((np.float16, ftk_amd.DTYPE_F16), (np.uint8, ftk_amd.DTYPE_U8), (np.int8, ftk_amd.DTYPE_I8), (np.uint16, ftk_amd.DTYPE_U16),
                        (np.int16, ftk_amd.DTYPE_I16), (np.uint32, ftk_amd.DTYPE_U32), (np.int32, ftk_amd.DTYPE_I32), (np.float32, ftk_amd.DTYPE_F32),
                        (np.float64, ftk_amd.DTYPE_F64)):
        a = np.zeros((5, 7), dtype=dtype)
        p, keep, dev, dt = ftk_amd._ptr_typed(a)
        assert p == a.ctypes.data and keep is a and dev == 0 and dt == code
    for bad in (np.int64, np.uint64, bool, np.complex64, np.dtype(">i2"), np.dtype(">f4")):
        with pytest.raises(TypeError):
            ftk_amd._ptr_typed(np.zeros(4, dtype=bad))
    with pytest.raises(TypeError):
        ftk_amd._one_dtype(ftk_amd.DTYPE_I16, ftk_amd.DTYPE_U8)
    assert ftk_amd._ptr(np.zeros(4, dtype=np.int32))[3] is False          # without keep_dtype: as before


def test_the_copy_of_a_view_lives_as_long_as_its_address():
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    view = img[..., 1]
    assert not view.flags.c_contiguous
    p, keep, dev, dt = ftk_amd._ptr_typed(view)
    assert keep is not view and keep.flags.c_contiguous and p == keep.ctypes.data and np.array_equal(keep, view)
    # the tracker's helper hands the copies on: the address it returns points into an array the caller holds
    h = Holder()
    ptrs, dev, dt, keeps = ftk_amd._TrackerRegular._narrow(h, True, None, view)
    assert dt == ftk_amd.DTYPE_U8 and dev == 0 and len(ptrs) == len(keeps) == 1
    assert keeps[0] is not None and keeps[0].flags.c_contiguous and ptrs[0] == keeps[0].ctypes.data and np.array_equal(keeps[0], view)
    assert h._keep == [None]                                               # nothing is kept beyond the call
    # three arrays of one push, one of them missing
    v16 = np.zeros((5, 7, 2, 2), dtype=np.int16)[..., 0]
    ptrs, dev, dt, keeps = ftk_amd._TrackerRegular._narrow(h, True, None, None, v16, None)
    assert ptrs[0] is None and ptrs[2] is None and ptrs[1] == keeps[1].ctypes.data and keeps[1].flags.c_contiguous
    # float32 / float64 and keep_dtype=False go the way they always went
    assert ftk_amd._TrackerRegular._narrow(h, True, None, np.zeros(4, dtype=np.float32)) is None
    assert ftk_amd._TrackerRegular._narrow(h, False, None, view) is None
    with pytest.raises(TypeError):
        ftk_amd._TrackerRegular._narrow(h, True, [np.zeros(4, dtype=np.uint8)], np.zeros(4, dtype=np.uint8))          # narrow extras are not taken
