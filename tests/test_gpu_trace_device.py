"""ftkx_trace_curves_device -- pass 2 with seeds, walks and compaction on the GPU as well (trace_order_kernels.hip) -- against the host
path ftkx_trace_curves, which tests/test_trace.py holds to the reference's finalize() point for point: the same curves in the same order,
every index sequence, every loop flag, the same count of special records."""
import numpy as np
import pytest

from trace_device_cases import FIXTURES, FRAGMENT_SEEDS, fixture_records, fragment, has_lone_point_and_two_point_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    import torch
    import ftk_amd
    assert torch.cuda.is_available()
    made = {}

    def get(nd):
        if nd not in made:
            made[nd] = ftk_amd.Context(nd)
        return made[nd]
    yield get
    for c in made.values():
        c.close()


def assert_same_curves(got, exp, what=""):
    (c2, l2, n2), (c1, l1, n1) = got, exp
    assert n2 == n1, what
    assert len(c2) == len(c1), what
    assert np.array_equal(np.asarray(l2), np.asarray(l1)), what
    assert np.array_equal(np.array([len(c) for c in c2]), np.array([len(c) for c in c1])), what
    if len(c1):
        assert np.array_equal(np.concatenate(c2), np.concatenate(c1)), what


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(ctxs, name):
    import ftk_amd
    g, dom, recs = fixture_records(name)
    ctx = ctxs(g["nd"])
    host = ftk_amd.trace_curves(g["nd"], dom, recs)
    for rep in range(2):                                   # (the second call reuses the context's buffers)
        dev = ftk_amd.trace_curves(g["nd"], dom, recs, ctx=ctx, device=True)
        assert ctx.trace_last_path() == 2
        assert_same_curves(dev, host, "%s, call %d" % (name, rep))
    if g["curves"] is not None:
        curves, loop, nspecial = dev
        got = sorted((tuple(recs["tag"][c].tolist()), int(l)) for c, l in zip(curves, loop))
        exp = sorted((tuple(t.tolist()), int(l)) for l, t in g["curves"])
        assert got == exp
        assert sum(len(c) for c in curves) + nspecial == len(recs)


@pytest.mark.parametrize("seed_index", range(8))
@pytest.mark.parametrize("p", [0.9, 0.5, 0.15])
@pytest.mark.parametrize("name", ["woven_31x37x32", "moving_extremum_3d_21x21x21x4_overflow"])
def test_fragmented_sets(ctxs, name, p, seed_index):
    """broken paths, curves of two points, lone points, opened cycles"""
    import ftk_amd
    g, dom, recs = fixture_records(name)
    ctx = ctxs(g["nd"])
    part = fragment(recs, p, FRAGMENT_SEEDS[(name, p)][seed_index])
    host = ftk_amd.trace_curves(g["nd"], dom, part)
    assert has_lone_point_and_two_point_loop(host[0], host[1])
    dev = ftk_amd.trace_curves(g["nd"], dom, part, ctx=ctx, device=True)
    assert ctx.trace_last_path() == 2
    assert_same_curves(dev, host)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
def test_tiny_sets(ctxs, n):
    """no size floor: the device form takes any n"""
    import ftk_amd
    g, dom, recs = fixture_records("woven_31x37x32")
    ctx = ctxs(g["nd"])
    host = ftk_amd.trace_curves(g["nd"], dom, recs[:n])
    dev = ftk_amd.trace_curves(g["nd"], dom, recs[:n], ctx=ctx, device=True)
    assert ctx.trace_last_path() == 2
    assert_same_curves(dev, host)
    assert sum(len(c) for c in dev[0]) + dev[2] == n


@pytest.mark.parametrize("name", ["woven_128x128x10", "moving_extremum_3d_21x21x21x4_overflow"])
def test_device_resident_tags(ctxs, name):
    import torch
    import ftk_amd
    g, dom, recs = fixture_records(name)
    ctx = ctxs(g["nd"])
    host = ftk_amd.trace_curves(g["nd"], dom, recs)
    tags = torch.from_numpy(np.ascontiguousarray(recs["tag"]).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = ftk_amd.trace_curves(g["nd"], dom, None, ctx=ctx, device=True, tags=tags)
    assert ctx.trace_last_path() == 2
    assert_same_curves(dev, host)
    # device-resident tags that are not ascending: noticed by the check kernel, traced the other way, same curves
    perm = np.random.default_rng(3).permutation(len(recs))
    shuffled = torch.from_numpy(np.ascontiguousarray(recs["tag"][perm]).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = ftk_amd.trace_curves(g["nd"], dom, None, ctx=ctx, device=True, tags=shuffled)
    assert ctx.trace_last_path() != 2
    assert_same_curves(dev, ftk_amd.trace_curves(g["nd"], dom, recs[perm]))


def test_fallbacks(ctxs):
    import ftk_amd
    g, dom, recs = fixture_records("woven_128x128x10")
    ctx = ctxs(g["nd"])
    perm = np.random.default_rng(5).permutation(len(recs))
    unsorted = recs[perm]
    dev = ftk_amd.trace_curves(g["nd"], dom, unsorted, ctx=ctx, device=True)
    assert ctx.trace_last_path() != 2
    assert_same_curves(dev, ftk_amd.trace_curves(g["nd"], dom, unsorted))
    twice = np.concatenate([recs[:10], recs[9:20]])
    with pytest.raises(ftk_amd.FtkxError):
        ftk_amd.trace_curves(g["nd"], dom, twice, ctx=ctx, device=True)
    ftk_amd.trace_curves(g["nd"], dom, recs, ctx=ctx, device=True)
    assert ctx.trace_last_path() == 2
    for part in (recs, recs[:100]):                        # without device=True: as before, the device phases (large sets) or the host
        got = ftk_amd.trace_curves(g["nd"], dom, part, ctx=ctx)
        assert ctx.trace_last_path() in (0, 1)
        assert_same_curves(got, ftk_amd.trace_curves(g["nd"], dom, part))


def test_pass2_on_device(ctxs):
    import ftk_amd
    g, dom, recs = fixture_records("woven_31x37x32")
    ctx = ctxs(g["nd"])
    c1, l1, n1, ts1, _a, _b = ftk_amd.pass2(g["nd"], dom, recs)
    c2, l2, n2, ts2, _a, _b = ftk_amd.pass2(g["nd"], dom, recs, ctx=ctx, device=True)
    assert ctx.trace_last_path() == 2
    assert_same_curves((c2, l2, n2), (c1, l1, n1))
    for f in ("offsets", "indices", "type", "t", "loop", "id"):
        assert np.array_equal(getattr(ts2, f), getattr(ts1, f)), f


def test_buffers_grow_shrink_and_change_dimension():
    """one context through calls of changing size and dimension: its pass-2 blocks are sized by bytes and shared by 2D (6 neighbour slots per
    record) and 3D (8) traces, so a block that a 3D call of 100 records sized is next addressed by a 2D call of 150; then calls that grow
    them, within the quarter of headroom and past it, small calls in large blocks, post-processing, and the trace with host walks"""
    import ftk_amd
    g3, dom3, recs3 = fixture_records("moving_extremum_3d_21x21x21x4_overflow")
    g2, dom2, recs2 = fixture_records("woven_31x37x32")
    gw, domw, recsw = fixture_records("woven_128x128x10")
    assert (g3["nd"], g2["nd"], gw["nd"]) == (3, 2, 2) and len(recs2) == 4491 and len(recsw) == 7357
    ctx = ftk_amd.Context(2)
    try:
        steps = [(3, dom3, recs3[:100]), (2, dom2, recs2[:150]), (2, dom2, recs2), (2, domw, recsw), (2, dom2, recs2[:150])]
        for k, (nd, dom, recs) in enumerate(steps):
            dev = ftk_amd.trace_curves(nd, dom, recs, ctx=ctx, device=True)
            assert ctx.trace_last_path() == 2, k
            assert_same_curves(dev, ftk_amd.trace_curves(nd, dom, recs), "step %d" % (k + 1))
        c1, l1, n1, ts1, _a, _b = ftk_amd.pass2(2, dom2, recs2)
        c2, l2, n2, ts2, _a, _b = ftk_amd.pass2(2, dom2, recs2, ctx=ctx, device=True, post_device=True)
        assert ctx.trace_last_path() == 2 and ctx.post_process_last_path() == 2
        assert_same_curves((c2, l2, n2), (c1, l1, n1), "step 6")
        for f in ("offsets", "indices", "type", "t", "loop", "id"):
            assert np.array_equal(getattr(ts2, f), getattr(ts1, f)), f
        got = ftk_amd.trace_curves(2, dom2, recs2, ctx=ctx)       # device phases, host walks: the same trace block
        assert ctx.trace_last_path() == 1
        assert_same_curves(got, (c1, l1, n1), "step 7")
    finally:
        ctx.close()


def test_tracker_traces_on_device():
    """a tracker over a small woven series, finalize() + post_process() with set_trace_on_device(True) and without: the same curves and
    trajectories; the first run's trace went all the way on the device"""
    import torch
    import ftk_amd
    from ftk_amd import synthetic
    assert torch.cuda.is_available()
    DW, DH, DT = 32, 32, 8
    steps = [synthetic.woven((DW, DH), k, DT, torch, "cuda") for k in range(DT)]
    torch.cuda.synchronize()
    runs = []
    for on_device in (True, False):
        tr = ftk_amd.CriticalPointTracker2DRegular()
        tr.set_scalar_field_source(ftk_amd.SOURCE_GIVEN); tr.set_vector_field_source(ftk_amd.SOURCE_DERIVED)
        tr.set_jacobian_field_source(ftk_amd.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
        tr.set_domain([2, 2], [DW - 3, DH - 3]); tr.set_array_domain([0, 0], [DW, DH])
        tr.set_tag_mode(ftk_amd.TAG_EXACT64)
        tr.initialize()
        tr.set_trace_on_device(on_device)
        for k in range(DT):
            tr.push_scalar_field_snapshot(steps[k])
            if k != 0:
                tr.advance_timestep()
            if k == DT - 1:
                tr.update_timestep()
        tr.finalize()
        path = tr.trace_last_path()
        curves, loop = tr.get_traced_critical_points()
        tr.post_process()
        trajs = tr.get_traced_trajectories()
        tr.close()
        runs.append((path, curves, loop, trajs))
    (p1, c1, l1, t1), (p0, c0, l0, t0) = runs
    assert p1 == 2 and p0 != 2
    assert sum(len(c) for c in c0) > 0
    assert len(c1) == len(c0) and np.array_equal(l1, l0)
    for a, b in zip(c1, c0):
        assert np.array_equal(a, b)
    assert len(t1) == len(t0)
    for a, b in zip(t1, t0):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
