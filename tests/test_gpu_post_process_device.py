"""ftkx_post_process_curves_device and ftkx_pass2_device -- trajectory post-processing as maps and scans on the GPU
(post_process_kernels.hip) -- against the host function ftkx_post_process_curves, which tests/test_trace.py holds to the reference's
json_interface::post_process on every fixture: the same trajectories field for field, t bit for bit."""
import numpy as np
import pytest

from post_process_cases import (FIXTURES, RUN_LENGTHS, SCRAMBLE_SEEDS, SCRAMBLED_FIXTURES, fixture_records, same_trajectories, scrambled,
                                shows_every_effect, traced)

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


def assert_same(got, exp, what=""):
    for f in ("offsets", "indices", "type", "loop", "id"):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), (what, f)
    assert np.array_equal(got.t.view(np.uint64), exp.t.view(np.uint64)), (what, "t")
    assert same_trajectories(got, exp)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(ctxs, name):
    import ftk_amd
    g, dom, recs = fixture_records(name)
    ctx = ctxs(g["nd"])
    host = ftk_amd.post_process(g["nd"], dom, recs)
    for rep in range(2):                                   # (the second call reuses the context's buffers)
        dev = ftk_amd.post_process(g["nd"], dom, recs, ctx=ctx, device=True)
        assert ctx.post_process_last_path() == 2
        assert_same(dev, host, "%s, call %d" % (name, rep))
    if g["pp"] is not None:
        got = sorted((tuple(recs["tag"][i].tolist()), tuple(ty.tolist()), tuple(tt.tolist()), lp) for i, ty, tt, lp in (dev.curve(c) for c in range(len(dev))))
        exp = sorted((tuple(tg.tolist()), tuple(ty.tolist()), tuple(tt.tolist()), lp) for lp, tg, ty, tt in g["pp"])
        assert got == exp


@pytest.mark.parametrize("seed_index", range(8))
@pytest.mark.parametrize("run_length", RUN_LENGTHS)
@pytest.mark.parametrize("name", SCRAMBLED_FIXTURES)
def test_scrambled_sets(ctxs, name, run_length, seed_index):
    """types drawn again in runs along the curves, ordinal bits redrawn, t jittered: smoothing, gaps, rotations, the alternating drop of
    split_all, reversals and both passes of adjust_time all over the set"""
    import ftk_amd
    g, dom, _ = fixture_records(name)
    ctx = ctxs(g["nd"])
    recs = scrambled(name, run_length, SCRAMBLE_SEEDS[(name, run_length)][seed_index])
    offs, flat, loop = traced(name)
    host = ftk_amd.post_process_curves(recs, offs, flat, loop)
    assert shows_every_effect(name, run_length, recs, host)
    dev = ftk_amd.post_process_curves(recs, offs, flat, loop, ctx=ctx, device=True)
    assert ctx.post_process_last_path() == 2
    assert_same(dev, host)


@pytest.mark.parametrize("name", ["merger_2d_32x32x100", "singular_terraces_72x64x56x8"])
def test_pass2_device_is_one_pipeline(ctxs, name):
    import ftk_amd
    g, dom, recs = fixture_records(name)
    ctx = ctxs(g["nd"])
    c1, l1, n1, ts1, _a, _b = ftk_amd.pass2(g["nd"], dom, recs)
    c2, l2, n2, ts2, _a, _b = ftk_amd.pass2(g["nd"], dom, recs, ctx=ctx, device=True, post_device=True)
    assert ctx.trace_last_path() == 2 and ctx.post_process_last_path() == 2
    assert n2 == n1 and len(c2) == len(c1) and np.array_equal(l2, l1)
    assert np.array_equal(np.concatenate(c2), np.concatenate(c1))
    assert np.array_equal([len(c) for c in c2], [len(c) for c in c1])
    assert_same(ts2, ts1, name)
    # the two halves apart, the curves going down and up again: the same
    c3, l3, n3, ts3, _a, _b = ftk_amd.pass2(g["nd"], dom, recs, ctx=ctx, device=True)
    c4, l4, n4, ts4, _a, _b = ftk_amd.pass2(g["nd"], dom, recs, ctx=ctx, post_device=True)
    assert ctx.post_process_last_path() == 2
    assert_same(ts3, ts1, name)
    assert_same(ts4, ts1, name)


A, B, CC = 1, 2, 4
TINY = [  # (types, offsets, loop flags) over six records
    ([], [0], []),                                          # no curves
    ([A], [0, 1], [0]),                                     # one curve of one point
    ([A, A], [0, 2], [1]),                                  # a loop of two points, equal types
    ([A, B], [0, 2], [1]),                                  # ... different types
    ([A, B, A], [0, 3], [0]),                               # split_all: B closes the first run and is dropped, the second A starts a run
    ([A, B, CC, CC], [0, 4], [0]),                          # ... B dropped, C kept with its run
    ([A, A, B, CC, A, A], [0, 6], [1]),                     # a loop that is rotated, then split
    ([A, B, CC, CC, A, B], [0, 0, 4, 4, 6, 6], [0, 0, 1, 1, 0]),   # empty curves between the others: empty trajectories
    ([0, 0, 0], [0, 3], [0]),                               # one type, and it is 0: split all the same
]


@pytest.mark.parametrize("case", range(len(TINY)))
@pytest.mark.parametrize("ordinals", [0, 0b000101, 0b111111])
def test_tiny(ctxs, case, ordinals):
    import ftk_amd
    types, offs, loop = TINY[case]
    ctx = ctxs(2)
    recs = np.zeros(6, dtype=ftk_amd.CP_DTYPE)
    recs["t"] = [0.5, 0.25, 0.75, 0.125, 0.875, 0.375]
    recs["type"][:len(types)] = types
    recs["aux"] = [((5 - k) << 1) | ((ordinals >> k) & 1) for k in range(6)]
    idx = np.arange(offs[-1])[::-1] if case % 2 else np.arange(offs[-1])
    host = ftk_amd.post_process_curves(recs, offs, idx, loop)
    dev = ftk_amd.post_process_curves(recs, offs, idx, loop, ctx=ctx, device=True)
    assert ctx.post_process_last_path() == 2
    assert_same(dev, host, str(TINY[case]))


def test_fallbacks(ctxs):
    import ftk_amd
    name = "merger_2d_32x32x100"
    g, dom, recs = fixture_records(name)
    ctx = ctxs(g["nd"])
    offs, flat, loop = traced(name)
    for bad in (np.nan, np.inf):                           # a t that is not finite, on a curve: the host does it, same result
        r = recs.copy()
        r["t"][flat[len(flat) // 2]] = bad
        host = ftk_amd.post_process_curves(r, offs, flat, loop)
        dev = ftk_amd.post_process_curves(r, offs, flat, loop, ctx=ctx, device=True)
        assert ctx.post_process_last_path() == 0
        for f in ("offsets", "indices", "type", "loop", "id"):
            assert np.array_equal(getattr(dev, f), getattr(host, f)), f
        assert np.array_equal(dev.t.view(np.uint64), host.t.view(np.uint64))
    beyond = flat.copy()
    beyond[3] = len(recs)
    with pytest.raises(ftk_amd.FtkxError):
        ftk_amd.post_process_curves(recs, offs, beyond, loop, ctx=ctx, device=True)
    descending = offs.copy()
    descending[1], descending[2] = descending[2], descending[1]
    assert descending[1] > descending[2]
    with pytest.raises(ftk_amd.FtkxError):
        ftk_amd.post_process_curves(recs, descending, flat, loop, ctx=ctx, device=True)
    dev = ftk_amd.post_process_curves(recs, offs, flat, loop, ctx=ctx, device=True)
    assert ctx.post_process_last_path() == 2
    assert_same(dev, ftk_amd.post_process_curves(recs, offs, flat, loop))


def test_tracker():
    """the 32 x 32 x 8 woven tracker of test_gpu_trace_device.py, finalize() + post_process() with trace and post-processing on the device
    against both off: the same trajectories, and the post-processing went all the way on the device"""
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
        tr.set_post_process_on_device(on_device)
        for k in range(DT):
            tr.push_scalar_field_snapshot(steps[k])
            if k != 0:
                tr.advance_timestep()
            if k == DT - 1:
                tr.update_timestep()
        tr.finalize()
        tr.post_process()
        path = tr.post_process_last_path()
        trajs = tr.get_traced_trajectories()
        tr.close()
        runs.append((path, trajs))
    (p1, t1), (p0, t0) = runs
    assert p1 == 2 and p0 == 0
    assert len(t1) == len(t0) and len(t0) > 0
    for a, b in zip(t1, t0):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
