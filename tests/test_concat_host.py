"""ftk_amd/csrc/concat_steps.hpp WITHOUT a GPU: the plan of a concat launch -- the common head peeled for alignment, the 16-byte body, the
vertex-wise variant where the planes disagree, the tail -- driven lane by lane through tests/hostcheck/concat_host.cpp (every element
written exactly once, nothing outside the array, the planes untouched, the value the widened float or the double's own bits), against the
numpy expression the GPU tests use as their oracle.  And the same file as a program of its own under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "concat_host.cpp")
UNTOUCHED = 0x7ff8dead0badbeef


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_concat.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.hc_concat.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.c_uint, C.c_void_p, C.POINTER(C.c_int)]
    L.hc_concat_group.argtypes = [C.c_int]
    return L


def values(dtype, nc, count, seed):
    """nc planes of every kind of value: random bit patterns (all exponents; NaNs of both signs and every payload, infinities) behind the named ones"""
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        named = np.array([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000], dtype=np.uint32)
        bits = rng.integers(0, 2 ** 32, size=nc * count, dtype=np.uint64).astype(np.uint32)
    else:
        named = np.array([0, 0x8000000000000000, 1, 0x8000000000000001, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000,
                          0x7ff0000000000001, 0xfff4000000abcdef, 0x7fefffffffffffff, 0x0010000000000000], dtype=np.uint64)
        bits = rng.integers(0, 2 ** 64, size=nc * count, dtype=np.uint64)
        bits[bits == UNTOUCHED] ^= 1
    k = min(bits.size, len(named))
    bits[:k] = named[:k]
    return bits.view(dtype).reshape(nc, count)


def oracle_bits(planes):
    """what the GPU tests hold the kernel to: numpy's interleave, then astype"""
    with np.errstate(invalid="ignore"):          # (a signalling NaN among the float bit patterns)
        return np.stack(list(planes), axis=-1).reshape(-1).astype(np.float64)


def offsets(G, nc):
    """(plane offsets, whether they agree): every common offset, and every way ONE plane can differ from it"""
    for o in range(G):
        yield [o] * nc, True
        for k in range(nc):
            for o2 in range(G):
                if o2 != o:
                    off = [o] * nc
                    off[k] = o2
                    yield off, False


@pytest.mark.parametrize("nc", (2, 3))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_every_element_once_and_nothing_else(hc, dtype, nc):
    f32 = int(dtype == np.float32)
    G = hc.hc_concat_group(f32)
    assert G == 16 // np.dtype(dtype).itemsize
    for count in list(range(0, 3 * G + 2)) + [255, 256, 257, 515]:
        x = values(dtype, nc, count, 1000 * count + 10 * nc + f32)
        exp = oracle_bits(x)
        nan = np.isnan(exp)
        for off, agree in offsets(G, nc):
            for dst_off in (0, 1):
                for nblocks in (1, 2, 3):
                    out = np.full(max(1, nc * count), 777.0)
                    vec = C.c_int(-1)
                    rc = hc.hc_concat(f32, nc, x.ctypes.data, count, (C.c_int * 3)(*(off + [0])[:3]), dst_off, nblocks, out.ctypes.data, C.byref(vec))
                    case = (dtype.__name__, nc, count, off, dst_off, nblocks)
                    assert rc == 0, (case, rc)
                    # the 16-byte body exactly where the planes agree and the destination falls on 16 bytes behind their head
                    head = (G - off[0]) % G
                    assert vec.value == int(agree and (dst_off + head * nc) % 2 == 0), case
                    got = out[:nc * count]
                    if f32:          # a NaN stays a NaN with its sign; which payload the conversion leaves is the hardware's
                        assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.signbit(got), np.signbit(exp)), case
                        assert np.array_equal(got.view(np.uint64)[~nan], exp.view(np.uint64)[~nan]), case
                    else:            # moved as bits
                        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), case


def test_the_planned_grid(hc):
    """nblocks 0: as many workgroups as the plan asks for (a lane per group below the cap)"""
    x = values(np.float32, 3, 3000, 5)
    out = np.zeros(9000)
    vec = C.c_int(-1)
    assert hc.hc_concat(1, 3, x.ctypes.data, 3000, (C.c_int * 3)(1, 1, 1), 1, 0, out.ctypes.data, C.byref(vec)) == 0
    assert vec.value == 1
    assert hc.hc_concat(1, 4, x.ctypes.data, 10, (C.c_int * 3)(0, 0, 0), 0, 0, None, None) == -1          # nc the kernel does not have


def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """(no skip where the runtimes are missing: the bounds of the planes and the destination are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of concat_steps.hpp cannot be made"
    exe = str(tmp_path / "concat_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DCONCAT_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "concat_host run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
