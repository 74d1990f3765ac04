"""The series of tests/one_launch_cases.py sit where tests/test_gpu_one_launch.py says they sit, checked WITHOUT a GPU: eligibility, nblocks and
nwg come from ftk_amd/csrc/one_plan.hpp -- the functions series.hip calls -- through tests/hostcheck/one_plan.cpp, the limits from
ftk_amd/csrc/sweep_params.hpp through the same program, and the keys a workgroup parks from the CPU oracle's records.  If a constant or
the geometry changes, the case that no longer sits on its edge fails here by name."""
import numpy as np
import pytest

import one_launch_cases as K


@pytest.fixture(scope="module")
def cases(oracle):
    return K.cases()


def _plan(c):
    p = c.plan()
    print(c.name, "n", c.n, "k", len(c.slice_ts), "cells", c.cells, p)
    return p


def test_the_plan_is_the_geometry_the_kernel_documents():
    """one_plan.hpp over sizes on both sides of every clamp: BS = 128 / 64, nblocks = ceil(cells * n / BS), nwg = max(8, min(256, (nblocks + 3) // 4)),
    and no workgroup of a pass that is taken owns more than kOneOwnBlocks blocks"""
    L = K.limits()
    assert (L["block2"], L["block3"]) == (128, 64)
    for nd in (2, 3):
        bs = 128 if nd == 2 else 64
        for cells, n in [(1, 1), (bs, 1), (bs + 1, 1), (63, 10), (27, 9), (bs * 28, 1), (bs * 29 - 1, 1), (bs * 32, 1), (bs * 32 + 1, 1), (bs * 1021, 1), (bs * 1024, 1), (bs * 1024 + 1, 1),
                         (bs * L["kOneMaxBlocks"] // 4, 4), (bs * L["kOneMaxBlocks"] // 4 + 1, 4)]:
            p = K.plan_of(nd, n, n + 1, cells, 1000)
            nblocks = -(-cells * n // bs)
            assert (p["nblocks"], p["nwg"], p["bs"]) == (nblocks, max(8, min(256, (nblocks + 3) // 4)), bs), (nd, cells, n, p)
            assert p["eligible"] == (nblocks <= L["kOneMaxBlocks"]), (nd, cells, n, p)
            if p["eligible"]:
                assert p["bpw"] <= L["kOneOwnBlocks"] and p["bpw"] * p["nwg"] >= nblocks, (nd, cells, n, p)
    assert L["kOneMaxBlocks"] == 256 * 32 and -(-L["kOneMaxBlocks"] // 256) <= L["kOneOwnBlocks"]


def test_eligibility_on_both_sides_of_each_limit():
    L = K.limits()
    S, SL = L["kOneMaxSteps"], L["kOneMaxSlices"]
    ok = lambda **kw: K.plan_of(**dict(dict(nd=2, n=4, k=5, cells=320, n_vertices=480, last_hits=0), **kw))["eligible"]      # noqa: E731
    assert ok(n=S, k=SL) and not ok(n=S + 1, k=SL) and not ok(n=S, k=SL + 1) and ok(n=1, k=1)
    assert ok(n_vertices=(1 << 22) // 5) and not ok(n_vertices=(1 << 22) // 5 + 1)
    assert ok(n=1, k=2, n_vertices=1 << 21) and not ok(n=2, k=3, n_vertices=1 << 21)
    # the hits rule: more than 2^17 corner-steps AND more than 2048 records in the context's last pass
    assert ok(cells=1 << 15, last_hits=10 ** 6) and ok(cells=(1 << 15) + 1, last_hits=2048) and not ok(cells=(1 << 15) + 1, last_hits=2049)


def test_key_store_full_and_one_over(cases):
    L = K.limits()
    full, over = cases["keys_full"], cases["keys_over"]
    for c, want, nrec in ((full, L["kOneKeys"], 1770), (over, L["kOneKeys"] + K.KEYS_OVER, 1764)):
        p = _plan(c)
        assert p == dict(eligible=True, nblocks=2048, nwg=256, bpw=8, bs=128) and c.cells == 128 * 128 and p["bpw"] * p["bs"] == 1024, (c.name, p)
        wg, _ = K.parked(c)
        r, f, _ = K.reference(c)
        print(c.name, "fullest", int(wg.max()), "in workgroup", int(wg.argmax()), "then", int(np.sort(wg)[-2]), "records", len(r))
        assert int(wg.max()) == want and int(wg.argmax()) == 85 and int(np.sort(wg)[-2]) < L["kOneKeys"], (c.name, int(wg.max()), int(np.sort(wg)[-2]))
        assert len(r) == nrec and set(f) == {256}, (c.name, len(r), f)
        assert len(r) <= 2048                    # (the hits rule does not bar the passes that follow on the same context)
    assert K.KEYS_OVER == 1
    again = cases["keys_over_again"]
    wg, _ = K.parked(again)
    assert _plan(again)["eligible"] and int(wg.max()) <= L["kOneKeys"] and len(K.reference(again)[0]) == 1764 and again.slices()[5].tobytes() == over.slices()[5].tobytes()


def test_block_limit(cases):
    L = K.limits()
    for nd in ("2d", "3d"):
        at, over = cases["blocks_%s_at" % nd], cases["blocks_%s_over" % nd]
        p, q = _plan(at), _plan(over)
        assert p["eligible"] and p["nblocks"] == L["kOneMaxBlocks"] and p["nwg"] == 256 and p["bpw"] == 32 and at.cells * at.n == L["kOneMaxBlocks"] * p["bs"], (at.name, p)
        assert not q["eligible"] and q["nblocks"] == L["kOneMaxBlocks"] + 1, (over.name, q)
        for c in (at, over):
            assert c.n <= L["kOneMaxSteps"] and c.n_vertices * len(c.slice_ts) <= 1 << 22      # (no other rule decides)
            r, f, _ = K.reference(c)
            wg, blk = K.parked(c)
            assert 0 < len(r) <= 2048 and int(wg.max()) <= L["kOneKeys"] and set(f) == {256}, (c.name, len(r))
            assert np.count_nonzero(blk) < len(blk) // 100, c.name                                # sparse: nearly every block is empty


def test_steps_and_slices(cases):
    L = K.limits()
    want = {"steps_47": (47, 48, True), "steps_48": (48, 48, False), "gapped_24": (24, 48, True), "gapped_25": (25, 50, False)}
    for name, (n, k, eligible) in want.items():
        c = cases[name]
        p = _plan(c)
        assert (c.n, len(c.slice_ts), p["eligible"]) == (n, k, eligible), (name, p)
        assert len(K.reference(c)[0]) > 0
    assert (L["kOneMaxSteps"], L["kOneMaxSlices"]) == (47, 48)
    assert cases["gapped_24"].slice_ts == list(range(48)) and cases["gapped_24"].ts == list(range(0, 48, 2))


def test_vertex_rule(cases, oracle):
    at, over = cases["vertices_at"], cases["vertices_over"]
    p, q = _plan(at), _plan(over)
    assert p["eligible"] and at.n_vertices * len(at.slice_ts) == 1 << 22 and len(at.slice_ts) == 2
    assert not q["eligible"] and len(over.slice_ts) == 3 and q["nblocks"] <= K.limits()["kOneMaxBlocks"]
    for d in range(2):                           # the core strictly inside the domain
        assert at.dom[0][d] < at.core[0][d] and at.core[0][d] + at.core[1][d] < at.dom[0][d] + at.dom[1][d]
    # the factor comes from far outside the core: the array as a whole gives 8192, a crop around the core 256
    r, f, res = K.reference(at)
    assert f == [8192] and len(r) > 0, f
    wg, _ = K.parked(at)
    assert int(wg.max()) <= K.limits()["kOneKeys"]
    a = at.slices()[0]
    V = oracle.gradient2D(a)
    crop = V[480:584, 980:1084]
    assert oracle.scaling_factor(oracle.resolution(crop))[0] == 256
    mag = np.abs(V)
    y, x = np.unravel_index(np.argmax(mag.max(axis=2)), mag.shape[:2])
    assert abs(int(x) - 2000) <= 1 and abs(int(y) - 1000) <= 1                        # the largest |v| is out there, too
    nz = np.where(mag == 0, np.inf, mag).min(axis=2)
    y, x = np.unravel_index(np.argmin(nz), nz.shape)
    assert abs(int(x) - 40) <= 1 and abs(int(y) - 30) <= 1


def test_straddling_blocks(cases):
    for name, nd, cells, bs in (("straddle_2d", 2, 63, 128), ("straddle_3d", 3, 27, 64)):
        c = cases[name]
        p = _plan(c)
        assert p["eligible"] and c.cells == cells < bs == p["bs"] and (cells * c.n) % bs != 0 and p["nblocks"] < p["nwg"] == 8, (name, p)     # a short last block, workgroups without a block
        r, _, _ = K.reference(c)
        steps_of_block = [set(range(b * bs // cells, min((b + 1) * bs - 1, cells * c.n - 1) // cells + 1)) for b in range(p["nblocks"])]
        assert all(len(s) >= 2 for s in steps_of_block), name                              # every block holds corners of two steps and more
        assert len(set(r["timestep"].tolist())) >= 2 * p["nblocks"] - 2, name                # records on both sides of the straddles
    c = cases["no_record"]
    assert _plan(c)["eligible"] and len(K.reference(c)[0]) == 0
    c = cases["one_record"]
    assert _plan(c)["eligible"] and len(K.reference(c)[0]) == 1 and c.n == 1


@pytest.mark.parametrize("name", ["plateau_2d", "plateau_3d"])
def test_degenerate_list_exactly_full(cases, oracle, name):
    """every vertex of the first block's corners has a zero vector in both slices: each round of G corners x NTYPES simplices fills s_deg[G * NTYPES]"""
    c = cases[name]
    p = _plan(c)
    assert p["eligible"] and c.scopes[0] == K.BOTH
    sl = c.slices()
    V = [K.derived(c, sl[t])[0] for t in (0, 1)]
    w = c.core[1]
    for lin in range(p["bs"]):                   # block 0: the first BS corners of step 0
        x = [lin % w[0], lin // w[0] % w[1]] + ([lin // (w[0] * w[1])] if c.nd == 3 else [])
        for corner in range(1 << c.nd):
            at = tuple(c.core[0][d] + x[d] + ((corner >> d) & 1) for d in reversed(range(c.nd)))
            assert not V[0][at].any() and not V[1][at].any(), (name, lin, at)
    assert any(v.any() for v in V) and len(K.reference(c)[0]) > 0      # (not the whole field: there are records behind the plateau)
    G, ntypes = 256 >> (c.nd + 1), 12 if c.nd == 2 else 60
    assert 4 * G == p["bs"] and G * ntypes == (384 if c.nd == 2 else 960)


def test_fragile_case_is_eligible_and_within_the_key_store(cases):
    """what the CPU can show of fragile_over: nothing but the fragile list can be too small (how many records are fragile is the GPU test's to say)"""
    c = cases["fragile_over"]
    wg, _ = K.parked(c)
    assert _plan(c)["eligible"] and c.nd == 3 and int(wg.max()) <= K.limits()["kOneKeys"] and 4096 < len(K.reference(c)[0]) <= 65536
    assert c.expect == K.limits()["SERIES_OVERFLOW"]


def test_scopes_and_other_ways_in(cases):
    for name in ("ordinal_only", "interval_only", "mixed_scopes", "image_bounds", "reference_tags", "work_index_tags", "degrees_2d", "vector_derived_j",
                 "vector_given_j", "offset_mesh"):
        c = cases[name]
        assert _plan(c)["eligible"], name
        r, f, _ = K.reference(c)
        assert len(r) > 0 and set(f) == {256}, (name, len(r), f)
    assert set(cases["ordinal_only"].scopes) == {K.ORDINAL} and len(cases["ordinal_only"].slice_ts) == 6
    assert set(cases["interval_only"].scopes) == {K.INTERVAL} and set(K.reference(cases["interval_only"])[0]["ordinal"].tolist()) == {0}
    assert set(K.reference(cases["ordinal_only"])[0]["ordinal"].tolist()) == {1}
    assert set(cases["mixed_scopes"].scopes) == {K.ORDINAL, K.INTERVAL, K.BOTH}
    c = cases["offset_mesh"]
    assert all(c.ext[0][d] > 0 and c.core[0][d] > c.dom[0][d] > c.ext[0][d] for d in range(2))
    assert cases["work_index_tags"].n == 1
    # records next to the array border and away from it in the same step: the straight-line gather of the record is not for the former
    c = cases["border_records"]
    r, _, _ = K.reference(c)
    assert _plan(c)["eligible"] and len(r) < 64
    for t in c.ts:
        xs = r["corner"][r["timestep"] == t][:, 0]
        assert xs.min() < 2 and 2 <= xs.max() < c.dims[0] - 3, (t, xs)
    c = cases["at_the_cap"]
    res = K.reference(c)[2]
    assert _plan(c)["eligible"] and set(res) == {2.0 ** -8} and set(K.reference(c)[1]) == {256}, res
    # image bounds change the coordinates, nothing else
    a, b = K.reference(cases["image_bounds"])[0], K.reference(cases["reference_tags"])[0]
    assert len(a) == len(b) and not np.array_equal(a["x"], b["x"])


def test_declines_the_kernel_raises(cases, oracle):
    L = K.limits()
    c = cases["inf"]
    assert _plan(c)["eligible"] and c.expect == L["SERIES_INF"] and sum(int(np.isinf(a).sum()) for a in c.slices().values()) == 1
    c = cases["ambiguous"]
    assert _plan(c)["eligible"] and c.expect == L["SERIES_AMBIGUOUS"]
    _, v = K.ambiguous_field(c.dims)
    frac = np.float64(1.0 / v).view(np.uint64) & np.uint64((1 << 52) - 1)
    assert 0 < int(frac) < (1 << 20), hex(int(frac))                                    # 1 / v just above 2^10
    r, f, res = K.reference(c)
    assert min(res) == v and set(f) == {2048} and len(r) > 0, (res, f)
