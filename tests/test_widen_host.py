"""ftk_amd/csrc/widen_steps.hpp WITHOUT a GPU: the plan of a widen launch -- the head peeled for alignment, the 16-byte body, the
element-wise variant, the tail -- driven lane by lane through tests/hostcheck/widen_host.cpp (every element written exactly once, nothing
outside the array, the value static_cast<double>), and the convolution's float-source staging against its double-source staging of the
widened array.  And the same file as a program of its own under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conv_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "widen_host.cpp")
COUNTS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025)


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_widen.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.hc_widen.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.hc_conv_f32.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hc_conv_f32.restype = C.c_long
    return L


def floats(count, seed):
    """every kind of float: random bit patterns (all exponents; NaNs and infinities among them) behind the named values"""
    named = np.array([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000], dtype=np.uint32)
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
    k = min(count, len(named))
    bits[:k] = named[:k]
    return bits.view(np.float32)


@pytest.mark.parametrize("count", COUNTS)
def test_every_element_once_and_nothing_else(hc, count):
    for src_off in range(4):
        for dst_off in range(2):
            x = floats(count, 100 * count + 10 * src_off + dst_off)
            out = np.full(max(1, count), 777.0)
            assert hc.hc_widen(x.ctypes.data, count, src_off, dst_off, out.ctypes.data) == 0, (count, src_off, dst_off)
            with np.errstate(invalid="ignore"):          # (a signalling NaN among the bit patterns)
                exp = x.astype(np.float64)
            nan = np.isnan(exp)
            assert np.array_equal(np.isnan(out[:count]), nan) and np.array_equal(np.signbit(out[:count]), np.signbit(exp))
            assert np.array_equal(out[:count].view(np.uint64)[~nan], exp.view(np.uint64)[~nan]), (count, src_off, dst_off)


@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_float_staging_is_the_double_staging_of_the_widened_array(hc, ksize):
    """every shape of the GPU tests, 2D and 3D: the tiles staged from the floats hold the bits of the tiles staged from the widened doubles"""
    for shape in CC.SHAPES_2D + CC.SHAPES_3D:
        a = CC.shape_input(shape, ksize).astype(np.float32)
        dims = list(shape) + [1] * (3 - len(shape))
        assert hc.hc_conv_f32(len(shape), ksize, a.ctypes.data, dims[0], dims[1], dims[2], None, None) == 0, (shape, ksize)


@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_float_source_convolution_against_the_restatement(hc, ksize):
    """... and what comes out of them is the convolution of the widened array (either side of the tile edges, Inf / NaN in range)"""
    for shape in [(33, 9), (9, 33), (65, 2), (2, 3), CC.INF_CASE_3D, CC.NAN_CASE_3D, (33, 9, 9), (2, 7, 1)]:
        a = CC.shape_input(shape, ksize).astype(np.float32)
        w = CC.gaussian_weights(len(shape), 0.75 + 0.25 * ksize, ksize)
        dims = list(shape) + [1] * (3 - len(shape))
        out = np.full(a.shape, 777.0)
        assert hc.hc_conv_f32(len(shape), ksize, a.ctypes.data, dims[0], dims[1], dims[2], w.ctypes.data, out.ctypes.data) == 0
        assert CC.same_bits(out, CC.conv(a.astype(np.float64), w)), (shape, ksize)


def test_sizes_the_kernel_does_not_have(hc):
    a = np.zeros((3, 3), dtype=np.float32)
    for nd, k in ((2, 4), (2, 0), (2, 11), (4, 3)):
        assert hc.hc_conv_f32(nd, k, a.ctypes.data, 3, 3, 1, None, None) == -1


def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """(no skip where the runtimes are missing: the bounds of the arrays and the tile are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of widen_steps.hpp cannot be made"
    exe = str(tmp_path / "widen_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DWIDEN_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "widen_host run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
