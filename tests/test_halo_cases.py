"""The premises of tests/test_gpu_halo_geometry.py, shown from the oracle and the mask plan alone, no GPU (tests/halo_cases.py): the cuts
are what tslab would make where tslab can make them, every case with summaries has a boundary whose request must hold cells, a 2D and a
3D boundary ask for more cells than a wavefront has lanes, the boundaries of the limit tests do not decline; the plain reference of the word
compaction on a hand-made summary array; the patch addresses at the core's first and last cell."""
import numpy as np
import pytest

import halo_cases as H
import mesh_cases as M
from test_mesh_cases import NAMES

SUMMARY = [f"{M._label(s[0], s[1])}_{p}" for s in M.SHAPES if s[5] for p in ("ragged", "aligned")] + ["3d_scalar_40x21x11_huge"]


@pytest.fixture(scope="module")
def cases(oracle):
    return M.cases()


@pytest.mark.parametrize("name", NAMES)
def test_the_cuts(cases, name):
    from ftk_amd import tslab
    c = cases[name]
    cuts = H.cuts(c)
    nt = c.n
    assert len(cuts) == (nt - 1) + (1 if nt >= 3 else 0) and len(set(cuts)) == len(cuts)
    assert sorted(cut[1] for cut in cuts if len(cut) == 3) == list(range(1, nt))          # one two-slab cut per interior slice boundary
    even = 0
    for cut in cuts:
        world = len(cut) - 1
        assert cut[0] == 0 and cut[-1] == nt and all(a < b for a, b in zip(cut, cut[1:]))          # no empty slab
        for t in range(nt):
            r = H.owner_of(cut, t)
            assert H.slab_range(cut, r)[0] <= t < H.slab_range(cut, r)[1]
        if all(H.slab_range(cut, r) == tslab.slab_range(nt, world, r) for r in range(world)):
            even += 1
            assert all(H.owner_of(cut, t) == tslab.owner_of(t, nt, world) for t in range(nt))
        # every boundary step is an interval step of the case, its halo a slice of the case
        for r, t in H.boundaries(cut):
            assert c.scopes[c.ts.index(t)] & M.INTERVAL and t + 1 in c.slice_ts and H.owner_of(cut, t + 1) == r + 1
        assert len(H.boundaries(cut)) == world - 1
    assert even >= 1                               # (tslab's own partition is among them: world 2 at nt // 2, world nt)
    if nt >= 3:
        assert any(len(cut) - 1 >= 3 for cut in cuts)          # a middle rank with both neighbours


@pytest.mark.parametrize("name", NAMES)
def test_the_per_step_counts_add_up(cases, name):
    """cull_counts_per_step against mesh_cases.cull_counts, whose result stays what it was: a step's cells once, removable under the
    interval's condition where the step has an interval scope (it implies the ordinal's), the ordinal's otherwise"""
    c = cases[name]
    per = H.cull_counts_per_step(c)
    assert len(per) == c.n
    cells = removable = 0
    for p, scope in zip(per, c.scopes):
        assert set(p) == ({M.ORDINAL, M.INTERVAL} if scope & M.INTERVAL else {M.ORDINAL})
        assert all(v[0] == c.cells and 0 <= v[1] <= v[0] for v in p.values())
        if scope & M.INTERVAL:
            assert p[M.INTERVAL][1] <= p[M.ORDINAL][1]
        cells += c.cells
        removable += p[M.INTERVAL if scope & M.INTERVAL else M.ORDINAL][1]
    assert (cells, removable) == M.cull_counts(c)


@pytest.mark.parametrize("name", SUMMARY)
def test_a_request_has_cells_it_must_hold(cases, name):
    c = cases[name]
    assert c.summaries
    seen = 0
    for cut in H.cuts(c):
        for r, t in H.boundaries(cut):
            L, Cc, R = H.request_bounds(c, t)
            assert 0 <= L <= Cc == c.cells and len(R) <= Cc and (len(R) == 0 or (R.min() >= 0 and R.max() < c.cells))
            assert len(np.unique(R)) == len(R)
            # a cell with an interval record cannot be one the strict-sign rule lets go
            assert len(R) <= L, (name, t, len(R), L)
            seen += len(R) > 0
    assert seen >= 1


def test_requests_cross_a_wavefront(cases):
    dims = set()
    for name in SUMMARY:
        c = cases[name]
        for cut in H.cuts(c):
            if any(H.must_decline(c, cut, r) for r in range(len(cut) - 1)):
                continue
            for r, t in H.boundaries(cut):
                if H.request_bounds(c, t)[0] >= 65:
                    dims.add(c.nd)
    assert dims == {2, 3}            # (the shapes of mesh_cases give both: no case was added)


def test_the_declining_slabs(cases):
    """the whole case needs the vertex rule exactly where one of its slabs does (every cut covers every step); the `huge` case declines
    everywhere; most cases decline nowhere"""
    declining = set()
    for name in NAMES:
        c = cases[name]
        for cut in H.cuts(c):
            slabs = [H.slab_needs_the_vertex_rule(c, cut, r) for r in range(len(cut) - 1)]
            assert any(slabs) == M.masks_need_the_vertex_rule(c), (name, cut, slabs)
            if any(H.must_decline(c, cut, r) for r in range(len(cut) - 1)):
                declining.add(name)
            if c.kind == "huge":
                assert all(H.must_decline(c, cut, r) for r in range(len(cut) - 1))
    assert "3d_scalar_40x21x11_huge" in declining and 2 <= len(declining) <= 6, declining
    assert [n for n in declining if n.endswith("_ragged")] == []


def test_the_limit_cases(cases):
    assert {cases[name].nd for name, _, _ in H.LIMIT_CASES} == {2, 3}
    for name, cut, t in H.LIMIT_CASES:
        c = cases[name]
        assert c.summaries and cut in H.cuts(c) and t in [b for _, b in H.boundaries(cut)]
        assert not any(H.must_decline(c, cut, r) for r in range(len(cut) - 1))
        L, Cc, R = H.request_bounds(c, t)
        assert 65 <= L <= Cc and len(R) > 0, (name, L, Cc)


@pytest.mark.parametrize("name", SUMMARY)
def test_the_plan_tells_the_rows_of_a_summary_byte(cases, name):
    c = cases[name]
    for env in (None, "1") + (("4",) if c.nd == 3 else ()):
        family, summaries, rows = M.planned(c, env, rows=True)
        assert summaries and (family, summaries) == M.planned(c, env)
        assert rows in (1, 4, 16) and (env is None or rows == int(env) or (env == "4" and rows in (1, 4))), (name, env, rows)


HAND = (20, 9)            # DW = 20: 3 groups, UP = 16, P = 32 (4 words a row); DH = 9: block rows of 4 -> 3, the last of one row


def _hand(nd, u_rows):
    """a summary array of 0xff with four zeros: in the last, clipped block row; in the last group; in the padding; (3D) in the second plane"""
    dims = HAND + ((2,) if nd == 3 else ())
    ngroups, UP, P, urows, DH, DD = H.summary_layout(dims, u_rows)
    assert (ngroups, UP, P, DH, DD) == (3, 16, 32, 9, nd - 1) and urows == {1: 9, 4: 3, 16: 1}[u_rows]
    U = np.full((DD, urows, UP), 0xff, dtype=np.uint8)
    U[0, urows - 1, 0] = 0            # the last block row: clipped at DH where u_rows does not divide 9
    U[0, 0, 2] = 0                    # the last group
    U[0, 0, 3] = 0                    # padding (g >= ngroups)
    U[0, urows - 1, UP - 1] = 0       # padding, the row's last byte
    if nd == 3:
        U[1, urows - 1, 1] = 0
    return dims, U


@pytest.mark.parametrize("nd", [2, 3])
def test_the_compaction_by_hand(nd):
    # u_rows = 1: a byte is one row
    dims, U = _hand(nd, 1)
    want = [8 * 4 + 0, 0 * 4 + 2] + ([(9 + 8) * 4 + 1] if nd == 3 else [])
    assert H.compacted(U, dims, 1).tolist() == sorted(want)
    # u_rows = 4: rows 8 .. 8 of the last block (clipped), rows 0 .. 3 of the first
    dims, U = _hand(nd, 4)
    want = [8 * 4 + 0] + [y * 4 + 2 for y in range(4)] + ([(9 + 8) * 4 + 1] if nd == 3 else [])
    assert H.compacted(U, dims, 4).tolist() == sorted(want)
    # u_rows = 16: one block row of 9 rows, both zeros in it
    dims, U = _hand(nd, 16)
    want = [y * 4 + 0 for y in range(9)] + [y * 4 + 2 for y in range(9)] + ([(9 + y) * 4 + 1 for y in range(9)] if nd == 3 else [])
    assert H.compacted(U, dims, 16).tolist() == sorted(want)
    # nothing to emit; everything to emit
    assert H.compacted(np.full(U.shape, 1, dtype=np.uint8), dims, 16).size == 0
    assert H.compacted(np.zeros(U.shape, dtype=np.uint8), dims, 16).tolist() == sorted(r * 4 + g for r in range(9 * (nd - 1)) for g in range(3))


@pytest.mark.parametrize("name", ["2d_scalar_40x23_ragged", "3d_scalar_40x21x11_aligned"])
def test_the_patch_addresses(cases, name):
    c = cases[name]
    at = H.patch_addresses(c, [0, c.cells - 1])
    assert at.shape == (2, 6 ** c.nd)
    first = [c.core[0][d] - c.ext[0][d] for d in range(c.nd)]
    last = [first[d] + c.core[1][d] - 1 for d in range(c.nd)]
    stride = np.cumprod([1] + list(c.dims[:-1]))
    # the patch's first element: corner - 2 on every axis; its last: corner + 3, clamped to the array
    assert at[0, 0] == sum((first[d] - 2) * stride[d] for d in range(c.nd))
    assert at[1, -1] == sum(min(last[d] + 3, c.dims[d] - 1) * stride[d] for d in range(c.nd))
    assert at.min() >= 0 and at.max() < c.n_vertices
    # (with the array at 0 and core = domain the same cells lie elsewhere: the origin and the core both show)
    z = M.at_origin_zero(c)
    assert np.array_equal(H.patch_addresses(z, [0, c.cells - 1]), at)          # relative to the array: a translation changes nothing
    w = M.whole_domain(c)
    assert not np.array_equal(H.patch_addresses(w, [0, c.cells - 1]), at)
