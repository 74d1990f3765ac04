"""What tests/test_adjust_host.py and tests/test_gpu_adjust.py share: the host build of ftk_amd/csrc/adjust_steps.hpp (tests/hostcheck/adjust_host.cpp,
a g++ shared object) as the oracle of the adjust kernel, the counts and offsets both walk, and inputs of every kind."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "adjust_host.cpp")
ROUND2 = 2048 * 256 * 2          # elements the capped grid takes in one round: behind it the grid-stride loop starts its second
COUNTS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, ROUND2 - 1, ROUND2, ROUND2 + 1)
MODES = {"clamp": (False, True), "perturb": (True, False), "both": (True, True)}
SIGMA, SEED, T, LO, HI = 0.25, 12345, 7, -1.0, 1.0

_lib = None


def host(tmp_dir=None):
    """the shared object, built once per process"""
    global _lib
    if _lib is None:
        import tempfile
        so = os.path.join(str(tmp_dir) if tmp_dir is not None else tempfile.mkdtemp(prefix="hostcheck_adjust"), "libhostcheck_adjust.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
        L = C.CDLL(so)
        vp, u64, sz = C.c_void_p, C.c_ulonglong, C.c_size_t
        L.hc_philox.argtypes = [vp, vp, vp]; L.hc_philox.restype = None
        L.hc_uniform.argtypes = [C.c_uint32, C.c_uint32]; L.hc_uniform.restype = C.c_double
        L.hc_ppnd16.argtypes = [vp, vp, sz]; L.hc_ppnd16.restype = None
        L.hc_log.argtypes = [vp, vp, sz]; L.hc_log.restype = None
        L.hc_clamp.argtypes = [vp, sz, C.c_double, C.c_double, vp]; L.hc_clamp.restype = None
        for f in (L.hc_adjust_f64, L.hc_adjust_f32):
            f.argtypes = [vp, sz, sz, C.c_int, C.c_double, u64, C.c_int, C.c_int, C.c_double, C.c_double, vp]; f.restype = None
        for f in (L.hc_plan_f64, L.hc_plan_f32):
            f.argtypes = [vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, u64, C.c_int, C.c_int, C.c_double, C.c_double, vp]
        _lib = L
    return _lib


def host_adjust(x, sigma=0.0, seed=0, t=0, clamp=None, e0=0):
    """the scalar function of (seed, t, e) over a flat array whose first element is element e0: float32 or float64 in, float64 out"""
    L = host()
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64)
    flat = x.reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    f = L.hc_adjust_f32 if x.dtype == np.float32 else L.hc_adjust_f64
    f(flat.ctypes.data, flat.size, int(e0), int(sigma > 0), float(sigma), int(seed), int(t), int(clamp is not None), float(lo), float(hi), out.ctypes.data)
    return out.reshape(x.shape)


NAMED64 = np.array([0, 1 << 63, 1, (1 << 63) | 1, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000, 0x7fefffffffffffff, 0xffefffffffffffff,
                    0x3ff0000000000000, 0xbff0000000000000, 0x3ff0000000000001, 0xbfefffffffffffff, 0x000fffffffffffff, 0x0010000000000000], dtype=np.uint64)
NAMED32 = np.array([0, 0x80000000, 1, 0x80000001, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f7fffff, 0xff7fffff, 0x3f800000, 0xbf800000, 0x3f800001, 0xbf7fffff,
                    0x007fffff, 0x00800000], dtype=np.uint32)


def values(count, seed, dtype):
    """+-0, subnormals, +-inf, quiet NaNs of either sign, +-max and the clamp's bounds with their neighbours in front; behind them three values
    in four lie in [-2, 2) -- around the bounds -1 and 1 -- and one in four is a random bit pattern (every exponent; NaNs of any payload are
    kept out: which payload an addition hands on is the hardware's business, and the quiet ones in front cover NaN in, NaN out)"""
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        bits = rng.integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
        x = bits.view(np.float32).copy()
        named = NAMED32.view(np.float32)
    else:
        bits = rng.integers(0, 2 ** 64, size=count, dtype=np.uint64)
        x = bits.view(np.float64).copy()
        named = NAMED64.view(np.float64)
    near = rng.uniform(-2.0, 2.0, size=count).astype(dtype)
    pick = rng.integers(0, 4, size=count)
    x = np.where((pick != 0) | np.isnan(x), near, x).astype(dtype)
    k = min(count, len(named))
    x[:k] = named[:k]
    return x


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
