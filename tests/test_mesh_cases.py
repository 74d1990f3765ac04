"""The cases of tests/mesh_cases.py are what they claim to be -- shown from the oracle and the mask plan alone, no GPU: the mesh is where
the table says, enough records lie in the core, some of the whole domain's lie outside it, every face of the core has one, both record
gathers are asked for, the partial words of a ragged core hold records; and the oracle itself commutes with a translation of the mesh."""
import numpy as np
import pytest

import mesh_cases as M

NAMES = [f"{M._label(s[0], s[1])}_{p}" for s in M.SHAPES for p in ("ragged", "aligned")] + ["3d_scalar_40x21x11_huge"]


@pytest.fixture(scope="module")
def cases(oracle):
    return M.cases()


def test_the_table(cases):
    assert sorted(cases) == sorted(NAMES)
    assert {c.family for c in cases.values()} == {s[3] for s in M.SHAPES} and len({s[3] for s in M.SHAPES}) == 9


@pytest.mark.parametrize("name", NAMES)
def test_the_mesh_is_where_it_should_be(cases, name):
    c = cases[name]
    org = M.ORIGIN[c.nd]
    assert org == [5, 7, 3][:c.nd] and list(c.ext[0]) == org and list(c.ext[1]) == list(c.dims)
    lo, cut = (2, 3) if c.nv == 1 else (1, 2)
    assert c.dom == ([o + lo for o in org], [d - cut for d in c.dims])
    for d in range(c.nd):          # the core strictly inside the domain on every face
        assert c.dom[0][d] < c.core[0][d] and c.core[0][d] + c.core[1][d] < c.dom[0][d] + c.dom[1][d], (name, d)
    first = c.core[0][0] - c.ext[0][0]
    last = first + c.core[1][0] - 1
    assert (first % 8, last % 8) == ((3, 4) if c.placement == "ragged" else (0, 7)), (first, last)
    assert 2 <= c.n <= 4 and c.scopes == [M.BOTH] * (c.n - 1) + [M.ORDINAL]
    if c.kind == "grid64":
        for a in c.slices().values():
            assert np.array_equal(a * 64.0, np.round(a * 64.0))


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_picks_the_family(cases, name):
    """plan_masks on the case's shape, through tests/hostcheck (the program tests/test_mask_plan.py drives)"""
    c = cases[name]
    assert M.planned(c) == (c.family, c.summaries), (name, M.planned(c))


@pytest.mark.parametrize("name", NAMES)
def test_the_records_a_case_needs(cases, name):
    c = cases[name]
    r, factors, _ = M.reference(c)
    assert len(r) >= 100, len(r)
    corner = r["corner"][:, :c.nd]
    for d in range(c.nd):
        assert corner[:, d].min() == c.core[0][d] and corner[:, d].max() == c.core[0][d] + c.core[1][d] - 1, (name, d)
    fast = M.is_fast_box(c, r)
    assert fast.any() and not fast.all()
    if c.placement == "ragged":
        x = M.array_rel(c, r)[:, 0]
        first, last = c.core[0][0] - c.ext[0][0], c.core[0][0] - c.ext[0][0] + c.core[1][0] - 1
        assert (x // 8 == first // 8).any() and (x // 8 == last // 8).any()
    if c.kind == "grid64":
        assert set(factors) == {256}
    # a kernel that ignores `core` and sweeps the domain gives other records
    w, _, _ = M.reference(M.whole_domain(c))
    inside = np.all((w["corner"][:, :c.nd] >= np.array(c.core[0])) & (w["corner"][:, :c.nd] < np.array(c.core[0]) + np.array(c.core[1])), axis=1)
    assert (~inside).any() and int(inside.sum()) == len(r)


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_commutes_with_a_translation(cases, name):
    """the same arrays swept at the origin 0 and at ORIGIN: tags (exact, relative to the domain), types, times and scalars equal, corners
    shifted by exactly the origin.  (x is not compared: it rounds differently; tests/test_offset_golden.py pins it.)"""
    c = cases[name]
    r, f, res = M.reference(c)
    z, fz, resz = M.reference(M.at_origin_zero(c))
    assert c.tag_mode == 2 and f == fz and res == resz and len(r) == len(z)
    for k in ("tag", "type", "etype", "t", "timestep", "ordinal"):
        assert np.array_equal(r[k], z[k]), k
    assert np.array_equal(r["scalar"], z["scalar"], equal_nan=True)
    shift = np.zeros(4, dtype=np.int64); shift[:c.nd] = c.origin
    assert np.array_equal(r["corner"].astype(np.int64), z["corner"].astype(np.int64) + shift)


@pytest.mark.parametrize("name", NAMES)
def test_the_cull_has_cells_to_drop_and_cells_to_keep(cases, name):
    """what tests/test_gpu_mesh_geometry.py asks of ctx.stats() is there to be had: the strict-sign cull, applied by hand to the oracle's
    gradients inside the core, drops some (step, corner) pairs and keeps others; in the `huge` case every vertex may wrap a determinant
    and nothing may be dropped"""
    c = cases[name]
    cells, removable = M.cull_counts(c)
    assert cells == c.cells * c.n
    if c.kind == "huge":
        assert removable == 0
    else:
        assert 0 < removable < cells, (cells, removable)


@pytest.mark.parametrize("name", ["2d_scalar_40x23_ragged", "3d_scalar_40x21x11_ragged"])
def test_the_aux_expectation_is_of_the_cases_records(cases, name):
    c = cases[name]
    r, _, _ = M.reference(c)
    e1, e2 = M.aux_expected(c, 0), M.aux_expected(c, 1)
    assert len(e1) == len(e2) == len(r) and not np.array_equal(e1, e2) and not np.array_equal(e1, r["scalar"][:, 0])
    assert np.abs(e1).max() <= 1e3
