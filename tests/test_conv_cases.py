"""The numpy restatement of the reference's spatial smoothing (tests/conv_cases.py) against what the reference itself wrote into
tests/golden/conv/: weights and outputs as uint64.  No GPU, no library."""
import numpy as np
import pytest

import conv_cases as CC


def test_there_are_fixtures():
    names = CC.fixture_names()
    assert len(names) >= 7
    assert {int(CC.load(n)["ksize"]) for n in names} >= {3, 5, 7, 9} and {int(CC.load(n)["nd"]) for n in names} == {2, 3}


@pytest.mark.parametrize("name", CC.fixture_names())
def test_restatement_equals_the_reference(name):
    f = CC.load(name)
    nd, sigma, ksize = int(f["nd"]), float(f["sigma"]), int(f["ksize"])
    assert f["input"].shape == tuple(reversed([int(d) for d in f["dims"]])) and f["output"].shape == f["input"].shape
    w = CC.gaussian_weights(nd, sigma, ksize)
    assert np.array_equal(w.view(np.uint64), f["weights"].view(np.uint64))
    assert np.array_equal(CC.conv(f["input"], f["weights"]).view(np.uint64), f["output"].view(np.uint64))
    assert np.array_equal(CC.conv_with_zeros(f["input"], f["weights"]).view(np.uint64), f["output"].view(np.uint64))
    # the inputs hold what they are meant to hold
    a = f["input"]
    assert (np.signbit(a) & (a == 0)).any() or a.size < 64
    assert ((a != 0) & (np.abs(a) < 1e-8)).any() or a.size < 64


def test_series_fixture():
    s = CC.series()
    DT = int(s["DT"])
    assert s["raw"].shape == s["smoothed"].shape == (DT, 37, 31)
    w = CC.gaussian_weights(2, float(s["sigma"]), int(s["ksize"]))
    assert np.array_equal(w.view(np.uint64), s["weights"].view(np.uint64))
    for k in range(DT):
        assert np.array_equal(CC.conv(s["raw"][k], w).view(np.uint64), s["smoothed"][k].view(np.uint64))


def test_shape_lists():
    assert len(CC.SHAPES_2D) == 105 and len(CC.SHAPES_3D) == 40
    for case in (CC.INF_CASE_2D, CC.NAN_CASE_2D):
        assert case in CC.SHAPES_2D
    assert np.isinf(CC.shape_input(CC.INF_CASE_3D, 3)).sum() == 2 and np.isnan(CC.shape_input(CC.NAN_CASE_3D, 3)).sum() == 1
    assert CC.same_bits(np.array([np.nan, -0.0]), np.array([np.nan, -0.0])) and not CC.same_bits(np.array([0.0]), np.array([-0.0]))
