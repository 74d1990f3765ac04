"""The long-chain sets of tests/trace_long_cases.py are what they claim to be, checked on the host trace WITHOUT a GPU: one open path and
one closed curve of at least 20 000 points each, and the path cut into pieces of 1, 2, 3, 16, 17, 256, 257, 4 096 and 4 097 points."""
import numpy as np

import trace_long_cases as T


def test_open_path():
    recs = T.records("open")
    curves, loop, nspecial = T.host_curves("open")
    assert len(curves) == 1 and len(curves[0]) >= T.MIN_POINTS and len(curves[0]) == len(recs) and loop[0] == 0 and nspecial == 0
    assert T.shows_what_it_must("open")
    steps = recs["aux"] >> 1
    assert steps.max() == T.OPEN_STEPS - 1 and steps.max() < (1 << 24)
    assert np.all(np.diff(recs["tag"].astype(np.uint64)) > 0)
    for a in range(2):                                     # the minimum where the field puts it, inside the domain all the way
        assert np.abs(recs["x"][:, a] - (T.OPEN_X0[a] + T.OPEN_V[a] * recs["t"])).max() < 1e-6
        assert recs["x"][:, a].min() > 3 and recs["x"][:, a].max() < (T.DW, T.DH)[a] - 4


def test_closed_curve():
    recs = T.records("closed")
    curves, loop, nspecial = T.host_curves("closed")
    assert len(curves) == 1 and len(curves[0]) >= T.MIN_POINTS and len(curves[0]) == len(recs) and loop[0] == 1 and nspecial == 0
    assert T.shows_what_it_must("closed")
    steps = recs["aux"] >> 1
    assert steps.min() > T.CLOSED_LEAD and steps.max() < T.CLOSED_STEPS - 1 - T.CLOSED_LEAD          # born and dies inside the series
    assert np.abs(recs["x"][:, 1] - T.CLOSED_X0[1]).max() < 1e-6
    assert recs["x"][:, 0].min() < T.CLOSED_X0[0] - 5 and recs["x"][:, 0].max() > T.CLOSED_X0[0] + 5   # both branches, far apart


def test_cut_sets():
    full, recs = T.records("open"), T.records("cut")
    assert len(recs) == len(full) - len(T.PIECES)
    curves, loop, nspecial = T.host_curves("cut")
    lens = sorted(len(c) for c in curves)
    assert lens == sorted(T.PIECES + [len(full) - sum(T.PIECES) - len(T.PIECES)]) and nspecial == 0
    assert T.shows_what_it_must("cut")
    assert [int(l) for c, l in zip(curves, loop) if len(c) != 2] == [0] * (len(curves) - 1)           # (a path of two points counts as a loop: cc2curves)
