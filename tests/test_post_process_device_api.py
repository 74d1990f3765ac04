"""The device form of the trajectory post-processing as the library and the package offer it; nothing here needs a GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

from post_process_cases import fixture_records, traced

NEW = ["ftkx_post_process_curves_device", "ftkx_pass2_device", "ftkx_post_process_last_path",
       "ftkx_tracker_set_post_process_on_device", "ftkx_tracker_post_process_last_path"]


def test_library_exports_the_new_functions():
    from ftk_amd import _lib, build
    build.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
    assert _lib.load().ftkx_post_process_last_path(None) == 0
    assert _lib.load().ftkx_post_process_curves_device(None, None, 0, None, None) == _lib.E_INVALID
    assert _lib.load().ftkx_pass2_device(None, 2, _lib.ll([0, 0]), _lib.ll([1, 1], fill=1), None, 0, None, None) == _lib.E_INVALID


def test_device_forms_need_a_context():
    import ftk_amd
    g, dom, recs = fixture_records("merger_2d_32x32x100")
    with pytest.raises(ValueError):
        ftk_amd.post_process(g["nd"], dom, recs, device=True)
    with pytest.raises(ValueError):
        ftk_amd.pass2(g["nd"], dom, recs, post_device=True)
    offs, flat, loop = traced("merger_2d_32x32x100")
    with pytest.raises(ValueError):
        ftk_amd.post_process_curves(recs, offs, flat, loop, device=True)
    # post_device is a keyword only: the positional signature bench.py calls stays
    params = inspect.signature(ftk_amd.pass2).parameters
    assert list(params)[:5] == ["nd", "domain", "records", "ctx", "device"]
    assert params["post_device"].kind is inspect.Parameter.KEYWORD_ONLY and params["post_device"].default is False
    for m in ("set_post_process_on_device", "post_process_last_path"):
        assert hasattr(ftk_amd.CriticalPointTracker2DRegular, m)
    assert hasattr(ftk_amd.Context, "post_process_last_path")


@pytest.mark.parametrize("name", ["merger_2d_32x32x100", "woven_31x37x32"])
def test_defaults_give_what_they_gave(name):
    import ftk_amd
    g, dom, recs = fixture_records(name)
    ts = ftk_amd.post_process(g["nd"], dom, recs)
    got = sorted((tuple(recs["tag"][i].tolist()), tuple(ty.tolist()), tuple(tt.tolist()), lp) for i, ty, tt, lp in (ts.curve(c) for c in range(len(ts))))
    exp = sorted((tuple(tg.tolist()), tuple(ty.tolist()), tuple(tt.tolist()), lp) for lp, tg, ty, tt in g["pp"])
    assert got == exp
    # the curves given as arrays: the same trajectories; and the 6-tuple of pass2
    offs, flat, loop = traced(name)
    again = ftk_amd.post_process_curves(recs, offs, flat, loop)
    for f in ("offsets", "indices", "type", "t", "loop", "id"):
        assert np.array_equal(getattr(again, f), getattr(ts, f)), f
    out = ftk_amd.pass2(g["nd"], dom, recs)
    assert len(out) == 6 and np.array_equal(out[3].indices, ts.indices)
