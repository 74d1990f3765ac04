"""How a vector snapshot under ftkx_set_vector_smoothing becomes the resident V, WITHOUT a GPU: every case of vec_smooth_ingest_plan
(ftk_amd/csrc/ingest_steps.hpp) through tests/hostcheck/vec_smooth_plan.cpp, held to the rules the interface states -- one kernel reads the
source and writes the slice, it reads this device's memory only, planes and floats get no launch of their own, on_device = 1 is read before
the call returns and never adopted, perturbation and clamp follow in place."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_vec_smooth_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "vec_smooth_plan.cpp")])
    L = C.CDLL(so)
    names = (C.c_int * 11)()
    L.hc_vec_smooth_names(names)
    return L, list(names)


def plan(L, f32, planar, adjust, on_device, here):
    out = (C.c_int * 8)()
    L.hc_vec_smooth_plan(int(f32), int(planar), int(adjust), on_device, int(here), out)
    return dict(zip(("reads_here", "adopt", "caller_waits", "stage", "copy", "first", "then_adjust", "counters"), out))


def test_every_case(hc):
    L, (ST_NONE, ST_F32, ST_POOLED, CP_NONE, CP_DST, CP_STAGE, CONV_VEC, IN_PLACE, VEC_INT, VEC_PLANAR, VEC_F32) = hc
    assert len({IN_PLACE, VEC_INT, VEC_PLANAR, VEC_F32}) == 4 and all(b & (b - 1) == 0 for b in (IN_PLACE, VEC_INT, VEC_PLANAR, VEC_F32))
    for f32, planar, adjust, on_device, here in itertools.product((0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)):
        p = plan(L, f32, planar, adjust, on_device, here)
        case = (f32, planar, adjust, on_device, here)
        asks = L.hc_vec_smooth_asks_where(planar, on_device)
        assert asks == int(on_device == 1 if planar else on_device != 0), case                      # planes of "any device" are always staged
        assert p["reads_here"] == int(asks and here), case
        assert p["adopt"] == 0, case                                                                 # the context owns the smoothed copy
        assert p["caller_waits"] == int(on_device != 0), case                                        # a device source has been read on return
        assert p["first"] == CONV_VEC and p["then_adjust"] == adjust, case                           # ONE kernel; the adjustment last, in place
        if p["reads_here"]:
            assert (p["stage"], p["copy"]) == (ST_NONE, CP_NONE), case
        else:
            assert (p["stage"], p["copy"]) == (ST_F32 if f32 else ST_POOLED, CP_STAGE), case       # never into dst: the kernel is out of place
        assert p["copy"] != CP_DST, case
        assert p["counters"] == (VEC_PLANAR if planar else VEC_INT) | (VEC_F32 if f32 else 0) | (IN_PLACE if adjust else 0), case
        if not asks:                                                                                  # where the pointers are not examined, they do not matter
            assert p == plan(L, f32, planar, adjust, on_device, 1 - here), case
