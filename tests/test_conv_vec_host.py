"""ftk_amd/csrc/conv_vec_steps.hpp WITHOUT a GPU: conv_vec_kernels.hip's loops -- per tile every component through one staged plane, from an
interleaved array or from planes, doubles or floats -- driven tile by tile through tests/hostcheck/conv_vec_host.cpp (g++,
-ffp-contract=off).  Held to the reference's own outputs with no new fixture: every file of tests/golden/conv/ fed as components
(S, 2 S[, S / 2]) must give (O, 2 O[, O / 2]) as 64-bit integers, since scaling by a power of two commutes with every rounding here (no
fixture output is zero or near the subnormal range).  Then all five sizes against the numpy restatement per component, and the same file
as a program of its own under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conv_cases as CC
import conv_vec_cases as VC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "conv_vec_host.cpp")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_conv_vec.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.hc_conv_vec.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hc_conv_vec_lds_bytes.argtypes = [C.c_int, C.c_int]
    return L


def host_conv_vec(L, V, w, planar=False, f32=False):
    """V: (..., nd) doubles (f32: representable as floats) -> the interleaved output"""
    nd = V.shape[-1]
    dt = np.float32 if f32 else np.float64
    if planar:
        keep = [np.ascontiguousarray(V[..., c], dtype=dt) for c in range(nd)]
    else:
        keep = [np.ascontiguousarray(V, dtype=dt)]
    ptrs = (C.c_void_p * 3)(*([a.ctypes.data for a in keep] + [None] * (3 - len(keep))))
    w = np.ascontiguousarray(w, dtype=np.float64)
    dims = list(reversed(V.shape[:-1])) + [1] * (3 - nd)
    out = np.full(V.shape, 777.0)
    assert L.hc_conv_vec(nd, w.shape[0], int(f32), int(planar), ptrs, dims[0], dims[1], dims[2], w.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("name", CC.fixture_names())
def test_fixtures_as_components(hc, name, planar):
    V, O = VC.fixture_vector(CC.load(name))
    got = host_conv_vec(hc, V, CC.load(name)["weights"], planar=planar)
    assert np.array_equal(got.view(np.uint64), O.view(np.uint64))


def test_scaling_by_a_power_of_two_commutes():
    """what the fixture check above rests on, shown with the restatement: conv(k S) == k conv(S) as bits for k = 2, 1 / 2, 4"""
    for name in CC.fixture_names():
        f = CC.load(name)
        assert np.abs(f["output"][f["output"] != 0]).min() > 1e-300 and (f["output"] != 0).all(), name
        for k in (2.0, 0.5, 4.0):
            assert np.array_equal(CC.conv(f["input"] * k, f["weights"]).view(np.uint64), (f["output"] * k).view(np.uint64)), (name, k)


@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_every_size_against_the_restatement(hc, ksize, planar, f32):
    for shape in VC.SHAPES_2D + VC.SHAPES_3D:
        V, clean = VC.shape_vector(shape, ksize, f32)
        w = VC.weights(len(shape), ksize)
        VC.check_against_restatement(host_conv_vec(hc, V, w, planar, f32), V, clean, w, (shape, ksize, planar, f32))


def test_sizes_the_kernel_does_not_have(hc):
    a = np.zeros((3, 3, 2)); w = np.zeros((4, 4)); o = np.zeros((3, 3, 2))
    ptrs = (C.c_void_p * 3)(a.ctypes.data, None, None)
    for nd, k in ((2, 4), (2, 0), (2, 11), (4, 3)):
        assert hc.hc_conv_vec(nd, k, 0, 0, ptrs, 3, 3, 1, w.ctypes.data, o.ctypes.data) == -1
        assert hc.hc_conv_vec_lds_bytes(nd, k) == -1


SANITIZED = [((6, 5), 7), ((1, 1), 9), ((2, 3), 5), ((4, 3, 3), 7), ((4, 3, 3), 9), ((1, 2, 1), 3), ((33, 33), 3), ((33, 9, 5), 5), ((31, 7, 9), 1), ((32, 32), 5), ((32, 8, 8), 3)]


def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """(no skip where the runtimes are missing: the bounds of the tile and of the arrays are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of conv_vec_steps.hpp cannot be made"
    exe = str(tmp_path / "conv_vec_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DCONV_VEC_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args, expected = [], []
    k = 0
    for shape, ksize in SANITIZED:
        for planar in (0, 1):
            for f32 in (0, 1):
                V, _ = VC.shape_vector(shape, ksize, bool(f32))
                nd = len(shape)
                w = CC.gaussian_weights(nd, 1.5, ksize)
                src = np.ascontiguousarray(np.moveaxis(V, -1, 0) if planar else V, dtype=np.float32 if f32 else np.float64)
                with open(tmp_path / ("in%d" % k), "wb") as f:
                    np.array([nd, ksize] + list(shape) + [1] * (3 - nd) + [f32, planar], dtype=np.int64).tofile(f)
                    w.tofile(f); src.tofile(f)
                args += [str(tmp_path / ("in%d" % k)), str(tmp_path / ("out%d" % k))]
                expected.append((VC.conv_vec(V, w), (shape, ksize, planar, f32)))
                k += 1
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "conv_vec_host run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    for k, (exp, what) in enumerate(expected):
        got = np.fromfile(tmp_path / ("out%d" % k), dtype=np.float64).reshape(exp.shape)
        assert CC.same_bits(got, exp), what
