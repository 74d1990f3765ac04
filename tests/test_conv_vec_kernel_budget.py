"""The vector smoothing's kernel at compile time (the method of tests/test_f32_kernel_budget.py: the compiler's kernel-resource-usage remarks
for the flags of the build): exactly the stated instantiations -- ND in {2, 3} x K in {1, 3, 5, 7, 9} x SRC in {double, float} -- and no
other, none with scratch, and each with the LDS that conv_vec_steps.hpp states (ConvVecTile::LDS_BYTES, asked of the header itself through
tests/hostcheck/conv_vec_host.cpp), which is the scalar kernel's: one staged plane."""
import ctypes as C
import os
import subprocess

import pytest

from test_f32_kernel_budget import HIPCC, resources

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("budget")
    return resources("conv_vec_kernels.hip", tmp), resources("conv_kernels.hip", tmp)


@pytest.fixture(scope="module")
def stated(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_conv_vec.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "conv_vec_host.cpp")])
    L = C.CDLL(so)
    L.hc_conv_vec_lds_bytes.argtypes = [C.c_int, C.c_int]
    return {(nd, k): L.hc_conv_vec_lds_bytes(nd, k) for nd in (2, 3) for k in (1, 3, 5, 7, 9)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_exactly_the_stated_instantiations(rows):
    want = {"ftkx::conv_vec_kernel<%d, %d, %s>" % (nd, k, t) for nd in (2, 3) for k in (1, 3, 5, 7, 9) for t in ("double", "float")}
    assert set(rows[0]) == want, sorted(set(rows[0]) ^ want)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_scratch_and_the_stated_lds(rows, stated):
    vec, scalar = rows
    for (nd, k), lds in sorted(stated.items()):
        assert 0 < lds <= 64 * 1024
        for t in ("double", "float"):
            name = "ftkx::conv_vec_kernel<%d, %d, %s>" % (nd, k, t)
            r = vec[name]
            print(name, r)
            assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
            assert int(r["LDS Size [bytes/block]"]) == lds, (name, r, lds)
            s = scalar["ftkx::conv_kernel<%d, %d, %s>" % (nd, k, t)]
            assert int(r["LDS Size [bytes/block]"]) == int(s["LDS Size [bytes/block]"]), (name, r, s)
            assert int(r["Occupancy [waves/SIMD]"]) >= int(s["Occupancy [waves/SIMD]"]), (name, r, s)      # the component loop costs no wave
