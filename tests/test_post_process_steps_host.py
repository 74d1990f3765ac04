"""ftk_amd/csrc/post_process_steps.hpp WITHOUT a GPU: post_process_steps() driven through tests/hostcheck/post_process_steps.cpp, once
with every scan as one left fold and once in the association of post_process_kernels.hip (eight items per thread, six doubling steps
over 64 lanes, four wave totals, tiles of 2 048 padded with identity(), the carry of the one-workgroup form, totals + spine + tiles above
8 192 points), against ftkx_post_process_curves: every field equal, t as uint64.  What this pins, whatever a GPU does: the operators are
associative, identity() is one on both sides, padding is harmless, and op(left, right) is kept at every level -- the sets of
tests/post_process_border_cases.py hold the -0.0 / 0.0 ties on which a swapped operand shows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import post_process_border_cases as B
from post_process_cases import FIXTURES, fixture_records, same_trajectories, traced

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "post_process_steps.cpp")
PP_RECORD = np.dtype([("type", "<u4"), ("aux", "<u4"), ("t", "<f8")])
SERIAL, TILED = 0, 1


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_pp_steps.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.hc_post_process_steps.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p] + [C.c_void_p] * 7
    L.hc_post_process_steps.restype = C.c_int
    return L


def packed(recs):
    out = np.zeros(len(recs), dtype=PP_RECORD)
    for f in ("type", "aux", "t"):
        out[f] = recs[f]
    return out


def steps(L, mode, recs, offs, indices, loop):
    import ftk_amd
    rec = packed(recs)
    offs = np.ascontiguousarray(offs, dtype=np.int64); indices = np.ascontiguousarray(indices, dtype=np.int64); loop = np.ascontiguousarray(loop, dtype=np.int32)
    nc = len(loop)
    n = int(offs[-1] - offs[0]) if nc else 0
    counts = np.zeros(2, dtype=np.int64)
    o_off = np.zeros(nc + n + 1, dtype=np.int64); o_loop = np.zeros(nc + n + 1, dtype=np.int32); o_id = np.zeros(nc + n + 1, dtype=np.int32)
    o_idx = np.zeros(n, dtype=np.int64); o_type = np.zeros(n, dtype=np.uint32); o_t = np.zeros(n, dtype=np.float64)
    rc = L.hc_post_process_steps(mode, rec.ctypes.data, len(rec), offs.ctypes.data, nc, indices.ctypes.data, len(indices), loop.ctypes.data,
                                 counts.ctypes.data, o_off.ctypes.data, o_idx.ctypes.data, o_type.ctypes.data, o_t.ctypes.data, o_loop.ctypes.data, o_id.ctypes.data)
    assert rc == 0, rc
    R, M = int(counts[0]), int(counts[1])
    return ftk_amd.TrajectorySet(o_off[:R + 1], o_idx[:M], o_type[:M], o_t[:M], o_loop[:R], o_id[:R])


def assert_same(got, exp, what):
    for f in ("offsets", "indices", "type", "loop", "id"):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), (what, f)
    assert np.array_equal(got.t.view(np.uint64), exp.t.view(np.uint64)), (what, "t")
    assert same_trajectories(got, exp)


@pytest.mark.parametrize("name", B.ALL)
def test_border_sets(hc, name):
    recs, offs, indices, loop, host = B.case(name)
    for mode in (SERIAL, TILED):
        assert_same(steps(hc, mode, recs, offs, indices, loop), host, (name, mode))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(hc, name):
    import ftk_amd
    _, _, recs = fixture_records(name)
    offs, flat, loop = traced(name)
    host = ftk_amd.post_process_curves(recs, offs, flat, loop)
    for mode in (SERIAL, TILED):
        assert_same(steps(hc, mode, recs, offs, flat, loop), host, (name, mode))


def test_tiny_and_empty(hc):
    """no curves, only empty curves, one point, and the tiny cases of the device test"""
    import ftk_amd
    A, Bt, CC = 1, 2, 4
    for types, offs, loop in [([], [0], []), ([], [0, 0, 0], [0, 1]), ([A], [0, 1], [0]), ([A, Bt, A], [0, 3], [0]), ([A, A, Bt, CC, A, A], [0, 6], [1]),
                              ([A, Bt, CC, CC, A, Bt], [0, 0, 4, 4, 6, 6], [0, 0, 1, 1, 0]), ([0, 0, 0], [0, 3], [0])]:
        recs = np.zeros(6, dtype=ftk_amd.CP_DTYPE)
        recs["t"] = [0.5, 0.25, 0.75, 0.125, 0.875, 0.375]
        recs["type"][:len(types)] = types
        recs["aux"] = [((5 - k) << 1) | ((0b000101 >> k) & 1) for k in range(6)]
        idx = np.arange(offs[-1])
        host = ftk_amd.post_process_curves(recs, offs, idx, loop)
        for mode in (SERIAL, TILED):
            assert_same(steps(hc, mode, recs, offs, idx, loop), host, (types, offs, mode))


def write_set(path, recs, offs, indices, loop):
    with open(path, "wb") as f:
        np.array([len(recs), len(loop), len(indices)], dtype=np.int64).tofile(f)
        packed(recs).tofile(f)
        np.ascontiguousarray(offs, dtype=np.int64).tofile(f); np.ascontiguousarray(indices, dtype=np.int64).tofile(f); np.ascontiguousarray(loop, dtype=np.int32).tofile(f)


def read_result(path):
    import ftk_amd
    with open(path, "rb") as f:
        R, M = (int(v) for v in np.fromfile(f, dtype=np.int64, count=2))
        offsets = np.fromfile(f, dtype=np.int64, count=R + 1); indices = np.fromfile(f, dtype=np.int64, count=M)
        ty = np.fromfile(f, dtype=np.uint32, count=M); t = np.fromfile(f, dtype=np.float64, count=M)
        loop = np.fromfile(f, dtype=np.int32, count=R); ident = np.fromfile(f, dtype=np.int32, count=R)
    return ftk_amd.TrajectorySet(offsets, indices, ty, t, loop, ident)


SANITIZED = [name for name, s in B.SETS.items() if s[1] == "257K+1"]


@pytest.mark.skipif(_runtime("libasan.so") is None or _runtime("libubsan.so") is None, reason="sanitizer runtimes not installed")
def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """the same file as a program of its own (no Python in the process), -fsanitize=address,undefined, once over the sets of 257K + 1
    points: both Run types, compared with each other there and with the host function here"""
    exe = str(tmp_path / "post_process_steps_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPP_STEPS_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args, expected = [], []
    for k, name in enumerate(SANITIZED):
        recs, offs, indices, loop, host = B.case(name)
        write_set(tmp_path / ("in%d" % k), recs, offs, indices, loop)
        args += [str(tmp_path / ("in%d" % k)), str(tmp_path / ("out%d" % k))]
        expected.append(host)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "post_process_steps run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    for k, name in enumerate(SANITIZED):
        assert_same(read_result(tmp_path / ("out%d" % k)), expected[k], name)
