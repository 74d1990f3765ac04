"""What tests/test_ingest_plan_host.py and tests/test_gpu_ingest_paths.py share: the host build of ftk_amd/csrc/ingest_steps.hpp
(tests/hostcheck/ingest_plan.cpp, a g++ shared object), the plan of a case with its enums by name, and the cases themselves."""
import collections
import ctypes as C
import itertools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "ingest_plan.cpp")
STAGES, COPIES, KERNELS = ("none", "f32_stage", "pooled"), ("none", "dst", "stage"), ("none", "concat", "conv", "adjust", "widen")
COUNTERS = ("from_float", "in_place", "out_of_place", "f32_widened", "f32_direct", "planar")
Plan = collections.namedtuple("Plan", "reads_here adopt caller_waits stage copy first then_adjust counters")

_lib = None


def host():
    """the shared object, built once per process; the enums' values are checked to be distinct and are turned into the names above"""
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="hostcheck_ingest"), "libhostcheck_ingest.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])
        L = C.CDLL(so)
        L.hc_ingest_plan.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)]; L.hc_ingest_plan.restype = None
        L.hc_ingest_asks_where.argtypes = [C.c_int] * 5
        L.hc_ingest_names.argtypes = [C.POINTER(C.c_int)]; L.hc_ingest_names.restype = None
        v = (C.c_int * 17)()
        L.hc_ingest_names(v)
        v = list(v)
        L.stage, L.copy, L.kernel = dict(zip(v[0:3], STAGES)), dict(zip(v[3:6], COPIES)), dict(zip(v[6:11], KERNELS))
        L.counter = dict(zip(v[11:17], COUNTERS))
        assert len(L.stage) == 3 and len(L.copy) == 3 and len(L.kernel) == 5 and len(L.counter) == 6
        assert all(b > 0 and b & (b - 1) == 0 for b in L.counter), "the counters are bits"
        _lib = L
    return _lib


def plan(f32, planar, smooth, adjust, on_device, on_this_device, must_own=False):
    """the header's plan of one case: enums by name, the counters as a frozenset of names"""
    L = host()
    o = (C.c_int * 8)()
    L.hc_ingest_plan(int(f32), int(planar), int(smooth), int(adjust), int(on_device), int(on_this_device), int(must_own), o)
    bits = int(o[7])
    assert bits & ~sum(L.counter) == 0
    return Plan(bool(o[0]), bool(o[1]), bool(o[2]), L.stage[o[3]], L.copy[o[4]], L.kernel[o[5]], bool(o[6]), frozenset(n for b, n in L.counter.items() if bits & b))


def asks_where(f32, planar, smooth, adjust, on_device):
    return bool(host().hc_ingest_asks_where(int(f32), int(planar), int(smooth), int(adjust), int(on_device)))


def all_inputs():
    """(f32, planar, smooth, adjust, on_device, on_this_device): all 96"""
    return list(itertools.product((False, True), (False, True), (False, True), (False, True), (0, 1, 2), (False, True)))
