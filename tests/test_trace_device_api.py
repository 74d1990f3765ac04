"""The public surface of the all-device trace (ftkx_trace_curves_device) as far as it can be checked without a GPU."""
import ctypes as C

import numpy as np
import pytest


def test_library_exports_the_device_trace():
    from ftk_amd import build, _lib
    build.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("ftkx_trace_curves_device", "ftkx_trace_last_path", "ftkx_tracker_set_trace_on_device"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def test_device_trace_needs_a_context():
    import ftk_amd
    from ftk_amd import build
    build.build()
    recs = np.zeros(3, dtype=ftk_amd.CP_DTYPE)
    recs["tag"] = [5, 17, 29]
    with pytest.raises(ValueError):
        ftk_amd.trace_curves(2, ([2, 2], [10, 10]), recs, device=True)
    with pytest.raises(ValueError):
        ftk_amd.pass2(2, ([2, 2], [10, 10]), recs, device=True)
    # without device=True nothing has changed: the host path
    curves, loop, nspecial = ftk_amd.trace_curves(2, ([2, 2], [10, 10]), recs)
    assert sum(len(c) for c in curves) + nspecial == 3
