"""ftk_amd/csrc/conv_steps.hpp WITHOUT a GPU: the tile, the staging, the lanes' places and the per-output arithmetic of conv_kernels.hip,
driven tile by tile through tests/hostcheck/conv_host.cpp (g++, -ffp-contract=off) and held to the reference's outputs in
tests/golden/conv/, bit for bit.  And the same file as a program of its own under AddressSanitizer + UBSan over arrays shorter than the
kernel and one array on either side of the tile edges: no read outside the input or the tile, no store outside the output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conv_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "conv_host.cpp")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_conv.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.hc_conv.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def host_conv(L, a, w):
    a = np.ascontiguousarray(a, dtype=np.float64); w = np.ascontiguousarray(w, dtype=np.float64)
    dims = list(reversed(a.shape)) + [1] * (3 - a.ndim)
    out = np.full(a.shape, 777.0)
    assert L.hc_conv(a.ndim, w.shape[0], a.ctypes.data, dims[0], dims[1], dims[2], w.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("name", CC.fixture_names())
def test_fixtures(hc, name):
    f = CC.load(name)
    assert np.array_equal(host_conv(hc, f["input"], f["weights"]).view(np.uint64), f["output"].view(np.uint64))


def test_series(hc):
    s = CC.series()
    for k in range(int(s["DT"])):
        assert np.array_equal(host_conv(hc, s["raw"][k], s["weights"]).view(np.uint64), s["smoothed"][k].view(np.uint64))


@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_every_size_against_the_restatement(hc, ksize):
    """all five sizes, 2D and 3D, on either side of the tile edges and with Inf / NaN in range"""
    for shape in [(33, 9), (9, 33), (65, 2), (2, 3), CC.INF_CASE_3D, CC.NAN_CASE_3D, (33, 9, 9), (2, 7, 1), (4, 3, 3)]:
        a = CC.shape_input(shape, ksize)
        w = CC.gaussian_weights(len(shape), 0.75 + 0.25 * ksize, ksize)
        assert CC.same_bits(host_conv(hc, a, w), CC.conv(a, w)), (shape, ksize)


def test_sizes_the_kernel_does_not_have(hc):
    a = np.zeros((3, 3)); w = np.zeros((4, 4))
    for nd, k in ((2, 4), (2, 0), (2, 11), (4, 3)):
        assert hc.hc_conv(nd, k, a.ctypes.data, 3, 3, 1, w.ctypes.data, a.ctypes.data) == -1


SANITIZED = [((6, 5), 7), ((1, 1), 9), ((2, 3), 5), ((4, 3, 3), 7), ((4, 3, 3), 9), ((1, 2, 1), 3), ((33, 33), 3), ((33, 9, 5), 5), ((31, 7, 9), 1)]


def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """(no skip where the runtimes are missing: the bounds of the tile and of the arrays are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of conv_steps.hpp cannot be made"
    exe = str(tmp_path / "conv_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DCONV_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args, expected = [], []
    for k, (shape, ksize) in enumerate(SANITIZED):
        a = CC.shape_input(shape, ksize)
        w = CC.gaussian_weights(len(shape), 1.5, ksize)
        with open(tmp_path / ("in%d" % k), "wb") as f:
            np.array([len(shape), ksize] + list(shape) + [1] * (3 - len(shape)), dtype=np.int64).tofile(f)
            w.tofile(f); a.tofile(f)
        args += [str(tmp_path / ("in%d" % k)), str(tmp_path / ("out%d" % k))]
        expected.append(CC.conv(a, w))
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "conv_host run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    for k, exp in enumerate(expected):
        got = np.fromfile(tmp_path / ("out%d" % k), dtype=np.float64).reshape(exp.shape)
        assert CC.same_bits(got, exp), SANITIZED[k]
