"""What Python does with the planes of a planar push before any call into the library (ftk_amd._planes), without a GPU: a sequence of nc
arrays or one (nc, ...) array becomes nc addresses with no copy made; a mix of dtypes or of host and device planes, planes of several
sizes, and anything that is not contiguous float32 / float64, is refused."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def planes():
    from ftk_amd import build
    build.build()          # (importing the package loads the library; hipcc cross-compiles it without a GPU)
    import ftk_amd
    return ftk_amd._planes


def test_a_sequence_and_a_stacked_array_are_read_where_they_lie(planes):
    for dtype in (np.float32, np.float64):
        u, v, w = (np.full((4, 5), k, dtype=dtype) for k in range(3))
        ptrs, nc, keep, dev, f32 = planes([u, v, w])
        assert (nc, dev, f32) == (3, 0, dtype == np.float32) and list(ptrs) == [a.ctypes.data for a in (u, v, w)]
        whole = np.zeros((2, 4, 5), dtype=dtype)
        ptrs, nc, keep, dev, f32 = planes(whole)
        assert (nc, dev, f32) == (2, 0, dtype == np.float32) and list(ptrs) == [whole.ctypes.data, whole.ctypes.data + whole[0].nbytes]
    ptrs, nc, keep, dev, f32 = planes((u, u))          # planes may be one another
    assert nc == 2 and ptrs[0] == ptrs[1]


def test_torch_planes(planes):
    import torch
    whole = torch.zeros((3, 2, 4, 5), dtype=torch.float32)
    ptrs, nc, keep, dev, f32 = planes(whole)
    assert (nc, dev, f32) == (3, 0, True) and list(ptrs) == [whole.data_ptr() + 160 * k for k in range(3)]
    with pytest.raises(TypeError):
        planes([torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.float16)])
    with pytest.raises(ValueError):
        planes(torch.zeros((2, 4, 6))[:, :, ::2])


def test_what_is_refused(planes):
    u, f = np.zeros((4, 5)), np.zeros((4, 5), dtype=np.float32)
    with pytest.raises(TypeError):
        planes([u, f])                                   # a mix of dtypes
    with pytest.raises(TypeError):
        planes([u.astype(np.int32), u.astype(np.int32)])
    with pytest.raises(TypeError):
        planes([u, [0.0] * 20])                          # not an array
    with pytest.raises(ValueError):
        planes([u, np.zeros((4, 6))])                    # several sizes
    with pytest.raises(ValueError):
        planes([u, np.zeros((4, 10))[:, ::2]])           # not contiguous: nothing is copied
    with pytest.raises(ValueError):
        planes(np.zeros((2, 4, 10))[:, :, ::2])
    with pytest.raises(ValueError):
        planes(np.zeros(20))                             # one array without a leading component axis
    with pytest.raises(ValueError):
        planes([])
