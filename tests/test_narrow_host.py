"""ftk_amd/csrc/narrow_steps.hpp WITHOUT a GPU: the conversion of one element of every narrow type -- over ALL bit patterns of the 8- and
16-bit types -- against numpy, and the plan of a narrow launch -- the head peeled for alignment, the 4-element body, the element-wise
variant, the tail -- driven lane by lane through tests/hostcheck/narrow_host.cpp (every element written exactly once, nothing outside the
array).  And the same file as a program of its own under AddressSanitizer + UBSan.

The yardstick: numpy's astype(float64) for the types numpy has (held to the reference's own from_array by tests/test_narrow_golden.py); for
bfloat16 the 16 bits moved to the top of a float32 word, then astype.  Everything is compared as 64-bit integers, NaNs by NaN-ness and sign."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "narrow_host.cpp")
COUNTS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025)
F16, BF16, U8, I8, U16, I16, U32, I32 = range(2, 10)          # FTKX_DTYPE_* (include/ftkx.h)
STORAGE = {F16: np.uint16, BF16: np.uint16, U8: np.uint8, I8: np.int8, U16: np.uint16, I16: np.int16, U32: np.uint32, I32: np.int32}
DTYPES = sorted(STORAGE)


def yardstick(dtype, stored):
    """what `stored` (the elements as numpy holds their bits) widens to"""
    with np.errstate(invalid="ignore"):          # (signalling NaNs among the bit patterns)
        if dtype == F16:
            return stored.view(np.float16).astype(np.float64)
        if dtype == BF16:
            return (stored.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return stored.astype(np.float64)


def assert_same(got, exp, what):
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.signbit(got), np.signbit(exp)), what
    assert np.array_equal(got.view(np.uint64)[~nan], exp.view(np.uint64)[~nan]), what


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_narrow.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.hc_narrow_one.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.hc_narrow.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.hc_narrow_grid.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    L.hc_narrow_form.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_int]
    L.hc_narrow_dtype_size.argtypes = [C.c_int]; L.hc_narrow_dtype_size.restype = C.c_size_t
    return L


def one(hc, dtype, stored):
    stored = np.ascontiguousarray(stored, dtype=STORAGE[dtype])
    out = np.full(len(stored), 777.0)
    assert hc.hc_narrow_one(dtype, stored.ctypes.data, len(stored), out.ctypes.data) == 0
    return out


def test_element_sizes(hc):
    assert [hc.hc_narrow_dtype_size(d) for d in range(-1, 12)] == [0, 8, 4, 2, 2, 1, 1, 2, 2, 4, 4, 0, 0]


@pytest.mark.parametrize("dtype", [F16, BF16, U16, I16])
def test_every_16_bit_pattern(hc, dtype):
    stored = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(STORAGE[dtype])
    exp = yardstick(dtype, stored)
    if dtype in (F16, BF16):          # the classes are all there: zeros, subnormals, normals, infinities, NaNs of both signs
        assert np.isnan(exp).sum() > 0 and np.isinf(exp).sum() == 2 and (exp == 0).sum() == 2 and np.signbit(exp[np.isnan(exp)]).any()
    if dtype == F16:
        assert exp[1] == 2.0 ** -24 and exp[0x03ff] == 1023 * 2.0 ** -24 and exp[0x0400] == 2.0 ** -14 and exp[0x7bff] == 65504.0
    assert_same(one(hc, dtype, stored), exp, dtype)


@pytest.mark.parametrize("dtype", [U8, I8])
def test_every_8_bit_pattern(hc, dtype):
    stored = np.arange(256, dtype=np.uint16).astype(np.uint8).view(STORAGE[dtype])
    assert_same(one(hc, dtype, stored), yardstick(dtype, stored), dtype)


def test_32_bit_integers(hc):
    named = np.array([0, 1, -1, -2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 31], dtype=np.int64)
    seeded = np.random.default_rng(32).integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.int64)
    bits = np.concatenate([named, seeded]).astype(np.uint64).astype(np.uint32)          # (the values as 32-bit patterns)
    for dtype in (U32, I32):
        stored = bits.view(STORAGE[dtype])
        exp = yardstick(dtype, stored)
        assert exp[5] == (2.0 ** 32 - 1 if dtype == U32 else -1.0) and exp[3] == (2.0 ** 31 if dtype == U32 else -2.0 ** 31)
        assert_same(one(hc, dtype, stored), exp, dtype)


def values(dtype, count, seed):
    """random bit patterns of the type (all its classes among them for a count of a few hundred)"""
    nbytes = np.dtype(STORAGE[dtype]).itemsize * count
    return np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8).view(STORAGE[dtype]) if count else np.zeros(0, dtype=STORAGE[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_once_and_nothing_else(hc, dtype):
    forms = set()
    for count in COUNTS:
        for src_off in range(4):
            for dst_off in range(2):
                x = values(dtype, count, 1000 * dtype + 100 * count + 10 * src_off + dst_off)
                out = np.full(max(1, count), 777.0)
                assert hc.hc_narrow(dtype, x.ctypes.data, count, src_off, dst_off, out.ctypes.data) == 0, (dtype, count, src_off, dst_off)
                assert_same(out[:count], yardstick(dtype, x), (dtype, count, src_off, dst_off))
                form = hc.hc_narrow_form(dtype, count, src_off, dst_off)
                assert form in (0, 1)
                # the 4-element body exactly when the head that aligns the source also brings the destination to 16 bytes (and fits)
                head = (4 - src_off) % 4
                assert form == (1 if head <= count and (head + dst_off) % 2 == 0 else 0), (dtype, count, src_off, dst_off)
                forms.add(form)
    assert forms == {0, 1}          # both the vector form and the element-wise form are hit


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_stride_loop_goes_round(hc, dtype):
    """fewer lanes than groups (a grid of 1 or 2 workgroups for up to 1250 groups): a lane takes two groups a turn, one grid apart, and the
    odd one at the end -- every element still exactly once"""
    for count in (1029, 2100, 5003):
        for grid in (1, 2):
            for src_off, dst_off in ((0, 0), (1, 1), (2, 0)):
                x = values(dtype, count, 7 * count + grid + src_off)
                out = np.full(count, 777.0)
                assert hc.hc_narrow_form(dtype, count, src_off, dst_off) == 1
                assert hc.hc_narrow_grid(dtype, x.ctypes.data, count, src_off, dst_off, grid, out.ctypes.data) == 0, (dtype, count, grid, src_off, dst_off)
                assert_same(out, yardstick(dtype, x), (dtype, count, grid, src_off, dst_off))


def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """(no skip where the runtimes are missing: the bounds of the arrays are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of narrow_steps.hpp cannot be made"
    exe = str(tmp_path / "narrow_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DNARROW_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "narrow_host run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
