"""Temporal Gaussian smoothing WITHOUT a GPU: the numpy restatement of the reference's filter (tests/temporal_cases.py), the library's
weights, and ftk_amd/csrc/temporal_steps.hpp -- the state machine and the per-element sum of temporal_kernels.hip -- as a program of its
own (tests/hostcheck/temporal_steps.cpp) under AddressSanitizer + UBSan, all held bit for bit to what the reference's own code gave
(tests/golden/temporal/)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import temporal_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "temporal_steps.cpp")
NEW = ["ftkx_gaussian_kernel1d", "ftkx_temporal_combine", "ftkx_set_temporal_smoothing", "ftkx_temporal_push", "ftkx_temporal_flush", "ftkx_debug_temporal_relaunch",
       "ftkx_tracker_set_temporal_smoothing", "ftkx_tracker_snapshots_from_last_push", "ftkx_tracker_flush_temporal_smoothing", "ftkx_tracker_reset"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def L():
    from ftk_amd import _lib, build
    build.build()
    return _lib.load()


def test_every_case_of_the_issue_has_its_fixture():
    assert set(TC.fixture_names()) == set(TC.EXPECTED_OUTPUTS)
    assert os.path.exists(os.path.join(TC.GOLDEN, TC.SERIES + ".npz"))


@pytest.mark.parametrize("name", sorted(TC.EXPECTED_OUTPUTS))
def test_restatement_equals_the_reference(name):
    f = TC.load(name)
    got = TC.smooth_series(list(f["input"]), f["weights"])
    assert len(got) == len(f["output"]) == TC.EXPECTED_OUTPUTS[name]
    for n, (g, e) in enumerate(zip(got, f["output"])):
        assert np.array_equal(bits(g), bits(e)), (name, n)
    if len(f["input"]) >= int(f["ksize"]):      # the closed form holds from N = K on
        for g, e in zip(TC.closed_form(list(f["input"]), f["weights"]), f["output"]):
            assert np.array_equal(bits(g), bits(e)), name


def test_restatement_equals_the_reference_on_the_series():
    s = TC.series()
    got = TC.smooth_series(list(s["raw"]), s["weights"])
    assert len(got) == int(s["DT"]) == 12
    assert np.array_equal(bits(np.stack(got)), bits(s["smoothed"]))
    assert not np.array_equal(bits(s["raw"]), bits(s["smoothed"]))


def test_library_exports_the_new_functions(L):
    from ftk_amd import _lib
    import ftk_amd
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(raw, name) is not None
        assert getattr(L, name).argtypes is not None, name
    for m in ("set_temporal_smoothing", "temporal_push", "temporal_flush", "temporal_combine"):
        assert hasattr(ftk_amd.Context, m)
    for m in ("set_temporal_smoothing", "snapshots_from_last_push", "flush_temporal_smoothing", "reset"):
        assert hasattr(ftk_amd.CriticalPointTracker2DRegular, m) and hasattr(ftk_amd.CriticalPointTracker3DRegular, m)
    assert "gaussian_kernel1d" in ftk_amd.__all__


@pytest.mark.parametrize("name", sorted(TC.EXPECTED_OUTPUTS) + [TC.SERIES])
def test_gaussian_kernel1d_is_the_references(L, name):
    """(the fixtures' weights come from the C library's exp of the machine that wrote them: this holds where that exp agrees)"""
    import ftk_amd
    f = TC.load(name)
    w = ftk_amd.gaussian_kernel1d(float(f["sigma"]), int(f["ksize"]))
    assert w.shape == f["weights"].shape
    assert np.array_equal(bits(w), bits(f["weights"]))
    assert np.array_equal(bits(TC.gaussian_weights(float(f["sigma"]), int(f["ksize"]))), bits(f["weights"]))


def test_argument_errors_without_a_gpu(L):
    from ftk_amd import _lib
    import ftk_amd
    w = np.zeros(16)
    for sigma, ksize in [(1.0, 4), (1.0, 2), (1.0, 0), (1.0, -3), (1.0, 11), (1.0, 10), (0.0, 3), (-1.0, 3), (float("nan"), 3), (float("inf"), 5), (float("-inf"), 5)]:
        assert L.ftkx_gaussian_kernel1d(sigma, ksize, w.ctypes.data) == _lib.E_INVALID, (sigma, ksize)
        with pytest.raises(ftk_amd.FtkxError):
            ftk_amd.gaussian_kernel1d(sigma, ksize)
    assert L.ftkx_gaussian_kernel1d(1.0, 3, None) == _lib.E_INVALID
    assert not w.any()
    buf = C.create_string_buffer(256)
    L.ftkx_gaussian_kernel1d(1.0, 4, w.ctypes.data)
    L.ftkx_last_error(None, buf, 256)
    assert b"ksize" in buf.value
    t = C.c_int(7)
    assert L.ftkx_set_temporal_smoothing(None, 1.0, 5, 0) == _lib.E_INVALID
    assert L.ftkx_temporal_push(None, w.ctypes.data, 0, 0, C.byref(t)) == _lib.E_INVALID
    assert L.ftkx_temporal_flush(None, C.byref(t)) == _lib.E_INVALID
    assert L.ftkx_temporal_combine(None, None, 3, w.ctypes.data, 4, None) == _lib.E_INVALID
    assert L.ftkx_tracker_set_temporal_smoothing(None, 1.0, 5) == _lib.E_INVALID
    assert L.ftkx_tracker_flush_temporal_smoothing(None, C.byref(t)) == _lib.E_INVALID


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """(no skip where the runtimes are missing: the bounds of the arrays are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of temporal_steps.hpp cannot be made"
    exe = str(tmp_path_factory.mktemp("hostcheck") / "temporal_steps_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _replay(exe, tmp_path, cases):
    """cases: (raw arrays, weights, offset) -> per case (emitted arrays, steps)"""
    args = []
    for k, (raw, w, offset) in enumerate(cases):
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        with open(tmp_path / ("in%d" % k), "wb") as f:
            np.array([len(w), raw.shape[0], raw[0].size if len(raw) else 4, offset], dtype=np.int64).tofile(f)
            np.ascontiguousarray(w, dtype=np.float64).tofile(f)
            raw.tofile(f)
        args += [str(tmp_path / ("in%d" % k)), str(tmp_path / ("out%d" % k))]
    assert "temporal_steps run complete" in _run(exe, ["run"] + args)
    res = []
    for k, (raw, w, offset) in enumerate(cases):
        with open(tmp_path / ("out%d" % k), "rb") as f:
            ne, ns = (int(v) for v in np.fromfile(f, dtype=np.int64, count=2))
            steps = np.fromfile(f, dtype=np.int64, count=ns * (2 + len(w))).reshape(ns, 2 + len(w))
            count = np.asarray(raw)[0].size if len(raw) else 4
            out = np.fromfile(f, dtype=np.float64, count=ne * count).reshape(ne, count)
        res.append((out, steps))
    return res


def test_steps_replay_the_fixtures_under_asan_ubsan(sanitized, tmp_path):
    """the header's state machine gives the restatement's index sequences, and its sum the reference's arrays: every fixture, short series
    included, on the 16-byte and on the 8-byte path"""
    names = sorted(TC.EXPECTED_OUTPUTS)
    cases, expect = [], []
    for name in names:
        f = TC.load(name)
        for offset in (0, 1):
            cases.append((f["input"].reshape(len(f["input"]), -1), f["weights"], offset))
            expect.append((name, f))
    for (name, f), (out, steps) in zip(expect, _replay(sanitized, tmp_path, cases)):
        assert len(out) == TC.EXPECTED_OUTPUTS[name], name
        assert np.array_equal(bits(out), bits(f["output"].reshape(len(f["output"]), out.shape[1]))), name
        trace = []
        TC.smooth_series(list(f["input"]), f["weights"], trace)
        want = [[0 if ph == "push" else 1, 0 if idx is None else 1] + (list(idx) if idx is not None else [-1] * int(f["ksize"])) for ph, idx in trace]
        assert steps.tolist() == want, name


def test_steps_on_odd_counts_and_more_than_one_grid_round(sanitized, tmp_path):
    """counts around the lane's two doubles and the workgroup's 512, and one above a whole capped grid (2048 workgroups of 256 lanes of two
    doubles), odd, so that the grid-stride loop's second round and the tail meet; Inf next to -Inf and a NaN in range"""
    cases, expect = [], []
    big = 2048 * 256 * 2 + 513
    for k, (ksize, n, count) in enumerate([(1, 2, 1), (3, 4, 2), (5, 6, 3), (7, 8, 255), (9, 10, 256), (5, 7, 257), (3, 5, 511), (5, 5, 513), (3, 4, big), (9, 3, 7)]):
        raw = TC.random_input((n, count), 100 + k)
        if count >= 255:
            raw[1, 5], raw[2, 5], raw[0, 9] = np.inf, -np.inf, np.nan
        w = TC.gaussian_weights(0.5 + 0.25 * ksize, ksize)
        for offset in ((0, 1) if count < big else (0,)):
            cases.append((raw, w, offset))
            expect.append(TC.smooth_series(list(raw), w))
    for (raw, w, offset), exp, (out, steps) in zip(cases, expect, _replay(sanitized, tmp_path, cases)):
        assert len(out) == len(exp), (len(w), raw.shape)
        if len(exp):
            assert TC.same_bits(out, np.stack(exp)), (len(w), raw.shape, offset)


def test_scalar_and_vector_snapshots_do_not_mix(sanitized):
    """temporal_admit is what ftkx_temporal_push asks: 0 admitted, 1 filter off, 2 mixed, 3 finishing"""
    out = _run(sanitized, ["admit"])
    assert "off=1 first=0 scalar_scalar=0 scalar_vector=2 vector_scalar=2 vector_vector=0 finishing=3 after=0" in out, out
