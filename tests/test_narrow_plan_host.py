"""ftk_amd/csrc/ingest_steps.hpp, narrow_ingest_plan, WITHOUT a GPU: how an array of halves, bfloat16s or 8- / 16- / 32-bit integers becomes
a resident FP64 array -- whether its bytes are staged, where the narrow kernel writes, whether the adjust kernel follows, whether the
caller waits -- for every case there is (smooth x adjust x on_device 0 / 1 / 2 x on_this_device), against the rules written out here a
second time.  ingest_plan itself is as it was (tests/test_ingest_plan_host.py)."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("reads_here", "staged", "adopt", "caller_waits", "to_pooled", "then_adjust", "counters")


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_narrow_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "narrow_plan.cpp")])
    return C.CDLL(so)


def plan(hc, smooth, adjust, on_device, on_this_device):
    out = (C.c_int * 7)()
    hc.hc_narrow_ingest_plan(int(smooth), int(adjust), on_device, int(on_this_device), out)
    return dict(zip(FIELDS, list(out)))


CASES = list(itertools.product((False, True), (False, True), (0, 1, 2), (False, True)))


def test_every_case(hc):
    bits = (C.c_int * 2)()
    hc.hc_narrow_counter_bits(bits)
    in_place, others = bits[0], bits[1]
    assert len(CASES) == 24
    for smooth, adjust, on_device, here in CASES:
        p = plan(hc, smooth, adjust, on_device, here)
        case = (smooth, adjust, on_device, here)
        # a kernel may read the caller's pointer only where the caller lends it (1) and it IS this device's memory: staged exactly otherwise
        may_read = on_device == 1 and here
        assert bool(p["reads_here"]) == may_read and bool(p["staged"]) == (not may_read), case
        assert p["adopt"] == 0, case                                                    # the resident array is FP64: never the caller's
        assert bool(p["caller_waits"]) == (on_device != 0), case                        # the float32 rule: a device source has been read on return
        assert bool(p["to_pooled"]) == smooth, case                                     # the pooled array exactly when the convolution follows
        assert bool(p["then_adjust"]) == adjust, case
        assert p["counters"] == (in_place if adjust else 0) and not (p["counters"] & others), case


def test_where_the_pointer_lies_is_asked_only_for_lent_memory(hc):
    assert [hc.hc_narrow_ingest_asks_where(d) for d in (0, 1, 2)] == [0, 1, 0]
    for smooth, adjust, on_device, _ in CASES:          # ... and where it is not asked, the answer does not matter
        if on_device != 1:
            assert plan(hc, smooth, adjust, on_device, False) == plan(hc, smooth, adjust, on_device, True)
