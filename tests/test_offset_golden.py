"""Pins the CPU oracle's handling of an array lattice that does not begin at the origin against the REAL reference: the fixtures under
tests/golden/offset/ were made by oracle/_ref/ftk_ref_driver with FTK_REF_ARRAY_START (tests/golden/make_golden_offset.py), which shifts
set_array_domain and set_domain by (5, 7[, 3]).  The oracle is assembled from pyoracle.sweep with (dom, core, ext) the way
one_launch_cases.reference does it -- pyoracle.track has no origin -- and must give the reference's records (tags as the reference
forms them, types, ordinal, timestep, x, t, scalar) and per-step factors bit for bit, with the lattice integers as coordinates and
with an image box (the reference divides v - array_start by array_size - 1)."""
import glob
import os

import numpy as np
import pytest

from common import GOLDEN, assert_records_equal
from one_launch_cases import BOTH, ORDINAL, Case, reference

NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "offset", "*.npz")))


def test_the_fixtures_are_there():
    assert len(NAMES) == 8 and sum(n.endswith("_bounds") for n in NAMES) == 4
    for n in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, "offset", n + ".npz")) < 2 ** 20


@pytest.mark.parametrize("name", NAMES)
def test_oracle_with_an_origin_matches_the_reference(oracle, name):
    z = np.load(os.path.join(GOLDEN, "offset", name + ".npz"))
    nd, nv, dims, DT = int(z["nd"]), int(z["nv"]), [int(d) for d in z["dims"]], int(z["DT"])
    start = [int(v) for v in z["array_start"]]
    assert start == [5, 7, 3][:nd]
    steps = z["steps"]
    lo, cut = (2, 3) if nv == 1 else (1, 2)           # oracle/ref_driver.cpp: set_domain
    dom = ([s + lo for s in start], [d - cut for d in dims])
    case = Case("golden_" + name, dims, range(DT), lambda t: steps[t], scopes=[BOTH] * (DT - 1) + [ORDINAL], nv=nv, ext_st=start, dom=dom,
                tag_mode=oracle.TAG_REFERENCE, bounds=[float(b) for b in z["bounds"]] if "bounds" in z.files else None)
    recs, factors, _ = reference(case)
    assert len(recs) > 1000
    assert np.array_equal(np.array(factors, dtype=np.uint64), z["factors"]), "per-step quantisation factor differs"
    assert recs["corner"][:, :nd].min(axis=0).tolist() >= dom[0]
    assert_records_equal(recs, z["records"], coord_tol=0.0, what=name)
