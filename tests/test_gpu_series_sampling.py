"""The series pass samples its own records (ftkx_set_series_sampling): scalar[1] / scalar[2] are filled by a kernel inside the device-driven
pass, in front of the records' copy to the host.  The armed pass returns what an unarmed pass followed by ftkx_sample_aux returns, byte for
byte -- plain, pipelined, split, with the slices and aux arrays dropped and pushed again under open passes, through every way out to the
host-driven batch --, the unarmed pass is not changed by the switch, and the trackers use it for deferred collection with components.
All comparisons of doubles are on bit patterns (a NaN equal to any NaN); records are compared as bytes."""
import numpy as np
import pytest

import sample_cases as SC
from common import load_golden
from test_gpu_aux import SMALL, make_context, make_tracker, only_slots_changed, push_fields, run_tracker_with, sweep_all

pytestmark = pytest.mark.gpu

PIPELINED = ("random_2d_scalar_29x24x6", "random_3d_scalar_13x12x11x4")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def same(a, b):
    return len(a) == len(b) and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def steps_of(gpu, g, t0=0):
    DT = g["DT"]
    return np.arange(t0, t0 + DT, dtype=np.int32), np.array([gpu.SCOPE_BOTH] * (DT - 1) + [gpu.SCOPE_ORDINAL], dtype=np.int32)


def armed(gpu, g, B, Cf, t0=0, **kw):
    ctx = make_context(gpu, g, t0=t0, **kw)
    ctx.set_series_sampling(True)
    push_fields(ctx, g, B, Cf, t0=t0)
    return ctx


_FIELDS = {}


def fields(name):
    if name not in _FIELDS:
        g = load_golden(name)
        _FIELDS[name] = ([SC.foreign_field(name, t, 0) for t in range(g["DT"])], [SC.foreign_field(name, t, 1) for t in range(g["DT"])])
    return _FIELDS[name]


_WANT = {}


def parents_way(gpu, name, t0=0, tag_mode=None, **kw):
    """an unarmed pass followed by ftkx_sample_aux, the foreign fields in both slots: computed once per (fixture, t0), handed out read-only"""
    key = (name, t0, tag_mode, tuple(sorted(kw.items())))
    if key not in _WANT:
        g = load_golden(name)
        B, Cf = fields(name)
        ctx = make_context(gpu, g, t0=t0, tag_mode=tag_mode, **kw)
        recs = sweep_all(gpu, ctx, g, t0=t0)
        push_fields(ctx, g, B, Cf, t0=t0)
        ctx.sample_aux(recs)
        assert ctx.series_sample_counts() == (0, 0, 0) and ctx.series_sampled() == (0, 0)
        ctx.close()
        recs.setflags(write=False)
        _WANT[key] = recs
    return _WANT[key]


# ---- 1. self-sampling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_own_scalar_field_comes_back_filled_from_the_pass(gpu, name, monkeypatch):
    g = load_golden(name)
    # the unarmed pass, held to the kernel chain (an armed pass with a slot to fill declines the one-launch form and the fused tail): whether
    # the chain itself covers this fixture, or raises a flag and leaves it to the host-driven batch (the overflow fixture: its masks need the
    # per-vertex rule), does not depend on the switch
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,small=0")
    plain = make_context(gpu, g)
    want = sweep_all(gpu, plain, g)
    device_driven = plain.series_last_path()[0] != 0
    plain.close()
    monkeypatch.delenv("FTKX_SERIES_HOOKS")
    ctx = armed(gpu, g, g["steps"], g["steps"])
    recs = sweep_all(gpu, ctx, g)
    print(name, len(recs), "records; unarmed path", "device" if device_driven else "host", "armed", ctx.series_last_path()[0], ctx.series_sampled(), ctx.series_sample_counts())
    assert len(recs) == len(g["records"]) > 0
    assert SC.same_doubles(recs["scalar"][:, 1], recs["scalar"][:, 0]) and SC.same_doubles(recs["scalar"][:, 2], recs["scalar"][:, 0])
    assert only_slots_changed(recs, want), "with the slots zeroed the records are those of an unarmed context"
    # a fixture whose options the device-driven form does not cover (a type filter, 3D without robust detection, flags raised by the kernels) is
    # swept by the host-driven batch with or without the switch: its records are filled behind the batch.  Every other one: by the kernel in the pass
    if device_driven:
        assert ctx.series_sampled() == (3, 1) and ctx.series_last_path()[0] == 1
        assert ctx.series_sample_counts()[:2] == (1, len(recs)) and ctx.sample_counts() == (0, 0)
    else:
        assert ctx.series_sampled() == (3, 2) and ctx.series_last_path()[0] == 0
        assert ctx.series_sample_counts()[1] == 0 and ctx.sample_counts() == (1, len(recs))
    ctx.close()


# ---- 2. foreign fields --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host_f64", "f32", "lent"])
@pytest.mark.parametrize("name", SC.FOREIGN)
def test_foreign_fields_armed_pass_equals_pass_plus_call_and_the_oracle(gpu, oracle, name, source):
    import torch
    g = load_golden(name)
    B, Cf = fields(name)
    if source == "f32":
        with np.errstate(over="ignore"):
            B1 = [b.astype(np.float32) for b in B]
        kw = {}
    elif source == "lent":
        B1 = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in B]
        Cd = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in Cf]
        torch.cuda.synchronize()
    else:
        B1 = B

    def push(ctx):
        for t in range(g["DT"]):
            if source == "lent":
                ctx.push_aux_slice(t, 1, B1[t], on_device=1); ctx.push_aux_slice(t, 2, Cd[t], on_device=1)
            else:
                ctx.push_aux_slice(t, 1, B1[t]); ctx.push_aux_slice(t, 2, Cf[t])

    plain = make_context(gpu, g)
    want = sweep_all(gpu, plain, g)
    push(plain)
    plain.sample_aux(want)
    plain.close()
    ctx = make_context(gpu, g)
    ctx.set_series_sampling(True)
    push(ctx)
    recs = sweep_all(gpu, ctx, g)
    assert ctx.series_sampled() == (3, 1) and ctx.series_last_path()[0] == 1
    assert same(recs, want), int((recs["scalar"][:, 1:].copy().view(np.uint64) != want["scalar"][:, 1:].copy().view(np.uint64)).sum())
    e2 = SC.expected_for(recs["tag"], SC.foreign_expectation(oracle, name, 1))
    assert SC.same_doubles(recs["scalar"][:, 2], e2)
    if source != "f32":
        assert SC.same_doubles(recs["scalar"][:, 1], SC.expected_for(recs["tag"], SC.foreign_expectation(oracle, name, 0)))
    ctx.close()


# ---- 3. pipelined, split and not, the arrays dropped and handed out again under open passes --------------------------------------------------
@pytest.mark.parametrize("split", [2, 0])
@pytest.mark.parametrize("name", PIPELINED)
def test_three_passes_in_flight_slices_and_aux_arrays_recycled(gpu, name, split, monkeypatch):
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,split=%d" % split)
    g = load_golden(name)
    DT, scalar = g["DT"], g["nv"] == 1
    B, Cf = fields(name)
    npass = 5
    t0s = [2 * DT * p for p in range(npass)]
    want = [parents_way(gpu, name, t0=t0, tag_mode=gpu.TAG_EXACT64) for t0 in t0s]
    ctx = armed(gpu, g, B, Cf, t0=t0s[0], tag_mode=gpu.TAG_EXACT64)
    done, paths = [], []

    def complete():
        r, _, _ = ctx.sweep_series_complete()
        done.append(r); paths.append(ctx.series_last_path()[0])
        assert ctx.series_sampled() == (3, 1), (len(done), ctx.series_sampled())

    for p, t0 in enumerate(t0s):
        if p:
            for k, a in enumerate(g["steps"]):
                (ctx.push_scalar_slice if scalar else ctx.push_slice)(t0 + k, a)
            push_fields(ctx, g, B, Cf, t0=t0)
        ctx.sweep_series_submit(*steps_of(gpu, g, t0))
        # every slice leaves with its aux arrays while the pass is open; the next pass's pushes take the arrays out of the pool again
        for k in range(DT):
            ctx.drop_slice(t0 + k)
        if p >= 2:
            complete()
    complete(); complete()
    print(name, "split", split, "paths", paths, "records", [len(r) for r in done])
    for p in range(npass):
        assert same(done[p], want[p]), (name, split, p, len(done[p]), len(want[p]))
    if split:
        assert all(q == 5 for q in paths[1:]), paths      # (the first pass of a context has no pass before it to be sparse)
    else:
        assert all(q == 1 for q in paths), paths
    assert ctx.series_sample_counts()[0] == npass and ctx.series_sample_counts()[1] == sum(len(r) for r in done)
    alloc, pooled = ctx.array_counts()
    assert pooled[0] == min(12, alloc[0]), (alloc, pooled)      # nothing is parked any more, nothing leaked: every field-class array is in the pool (its cap: 12) or freed
    ctx.close()


# ---- 4. the stride loop on the device -------------------------------------------------------------------------------------------------------------
def test_more_records_than_lanes_on_a_fresh_context_and_a_pass_without_records(gpu, monkeypatch):
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0")
    name = "woven_128x128x10"
    g = load_golden(name)
    plain = make_context(gpu, g, tag_mode=gpu.TAG_EXACT64)
    want = sweep_all(gpu, plain, g)
    plain.close()
    ctx = armed(gpu, g, g["steps"], g["steps"], tag_mode=gpu.TAG_EXACT64)      # fresh: the grid comes from a hit count of 0
    recs = sweep_all(gpu, ctx, g)
    launches, records, wgs = ctx.series_sample_counts()
    print(name, "records", len(recs), "workgroups", wgs)
    assert launches == 1 and records == len(recs) and len(recs) > wgs * 256, (launches, records, wgs, len(recs))
    assert ctx.series_sampled() == (3, 1) and only_slots_changed(recs, want)
    assert SC.same_doubles(recs["scalar"][:, 1], recs["scalar"][:, 0]) and SC.same_doubles(recs["scalar"][:, 2], recs["scalar"][:, 0])
    ctx.close()
    # a pass whose steps yield no record: a ramp has no critical point
    dims = (40, 33)
    ramp = [np.ascontiguousarray(np.add.outer(2.0 * np.arange(dims[1]), 1.0 * np.arange(dims[0])) + 0.25 * t) for t in range(3)]
    ctx = gpu.Context(2)
    dom = ([2, 2], [d - 3 for d in dims])
    ctx.set_mesh(dom, dom, ([0, 0], list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_EXACT64)
    ctx.set_series_sampling(True)
    for t, a in enumerate(ramp):
        ctx.push_scalar_slice(t, a); ctx.push_aux_slice(t, 1, a)
    recs, _, _ = ctx.sweep_series([0, 1, 2], [gpu.SCOPE_BOTH, gpu.SCOPE_BOTH, gpu.SCOPE_ORDINAL])
    assert len(recs) == 0 and ctx.series_sampled() == (1, 1) and ctx.series_last_path()[0] == 1 and ctx.series_sample_counts()[:2] == (1, 0)
    ctx.close()


# ---- 5. ways out ------------------------------------------------------------------------------------------------------------------------------------
def test_ways_out_to_the_host_driven_batch_fill_the_records_too(gpu, monkeypatch):
    name = "random_2d_scalar_29x24x6"
    g = load_golden(name)
    B, Cf = fields(name)
    want = parents_way(gpu, name)
    # the form switched off
    monkeypatch.setenv("FTKX_SERIES", "0")
    ctx = armed(gpu, g, B, Cf)
    recs = sweep_all(gpu, ctx, g)
    assert ctx.series_sampled() == (3, 2) and ctx.series_last_path()[0] == 0 and same(recs, want)
    assert ctx.series_sample_counts() == (0, 0, 0) and ctx.sample_counts() == (1, len(recs))
    ctx.close()
    monkeypatch.delenv("FTKX_SERIES")
    # exact_only: not the device-driven form
    ctx = armed(gpu, g, B, Cf, exact_only=True)
    recs = sweep_all(gpu, ctx, g)
    assert ctx.series_sampled() == (3, 2) and ctx.series_last_path()[0] == 0 and same(recs, parents_way(gpu, name, exact_only=True))
    ctx.close()
    # buckets too full to rank on the device: the host orders the records, which are filled already
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,rank_max=0")
    ctx = armed(gpu, g, B, Cf)
    recs = sweep_all(gpu, ctx, g)
    p = ctx.series_last_path()
    assert p[0] == 1 and (p[1] & 16) and ctx.series_sampled() == (3, 1), p
    assert np.all(recs["tag"][1:] > recs["tag"][:-1]) and same(recs, want)
    ctx.close()


def test_overflow_replay_is_filled_behind_the_batch_and_the_next_call_in_the_pass(gpu, monkeypatch):
    """the shape of test_gpu_series.py::test_series_overflowing_buffers_replays_through_the_batch: more records than the initial hit buffer holds"""
    from ftk_amd import synthetic
    import torch
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0")
    dims, nt = (2048, 2048), 12
    ctx = gpu.Context(2)
    dom = ([2, 2], [d - 3 for d in dims])
    ctx.set_mesh(dom, dom, ([0, 0], list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_EXACT64)
    ctx.set_series_sampling(True)
    dev = torch.device("cuda", 0)
    keep = []
    for t in range(nt):
        s = synthetic.generate("woven", dims, t, nt, torch, dev); keep.append(s)
        torch.cuda.synchronize()
        ctx.push_scalar_slice(t, s)
        ctx.push_aux_slice(t, 1, s, on_device=1); ctx.push_aux_slice(t, 2, s, on_device=1)      # lent: the snapshot itself
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    r1, f1, _ = ctx.sweep_series(range(nt), scopes)
    p1 = ctx.series_last_path()
    assert len(r1) > 65536, len(r1)
    assert p1[0] == 0 and (p1[1] & 8) and ctx.series_sampled() == (3, 2), (p1, ctx.series_sampled())
    ctx.invalidate_masks()
    r2, f2, _ = ctx.sweep_series(range(nt), scopes)
    assert ctx.series_last_path()[0] == 1 and ctx.series_sampled() == (3, 1), (ctx.series_last_path(), ctx.series_sampled())
    assert same(r1, r2) and np.array_equal(f1, f2)
    assert SC.same_doubles(r2["scalar"][:, 1], r2["scalar"][:, 0]) and SC.same_doubles(r2["scalar"][:, 2], r2["scalar"][:, 0]) and r2["scalar"][:, 0].view(np.uint64).any()
    ctx.close()


# ---- 6. contract ----------------------------------------------------------------------------------------------------------------------------------
def code(gpu, f):
    with pytest.raises(gpu.FtkxError) as e:
        f()
    return e.value.code


def test_contract(gpu, monkeypatch):
    import torch
    name = "random_2d_scalar_29x24x6"
    g = load_golden(name)
    DT = g["DT"]
    B, Cf = fields(name)
    ts, scopes = steps_of(gpu, g)
    want = parents_way(gpu, name)
    # a slot at some but not all of the timesteps: -4, nothing queued, the context stays usable
    ctx = make_context(gpu, g)
    ctx.set_series_sampling(True)
    push_fields(ctx, g, B, None)
    for t in range(DT - 1):
        ctx.push_aux_slice(t, 2, Cf[t])
    assert code(gpu, lambda: ctx.sweep_series(ts, scopes)) == -4
    assert code(gpu, lambda: ctx.sweep_series_submit(ts, scopes)) == -4
    assert ctx.series_sample_counts() == (0, 0, 0)
    # ... the steps that do not read the last slice are fine (slot 2 included), and so is the whole pass once the array is there
    r, _, _ = ctx.sweep_series(ts[:DT - 2], scopes[:DT - 2])
    assert ctx.series_sampled() == (3, 1) and same(r, want[(want["aux"] >> 1) < DT - 2])
    ctx.push_aux_slice(DT - 1, 2, Cf[DT - 1])
    ctx.invalidate_masks()
    r, _, _ = ctx.sweep_series(ts, scopes)
    assert ctx.series_sampled() == (3, 1) and same(r, want)
    # the switch with a pass open: -1; the pass completes as it was submitted
    ctx.invalidate_masks()
    ctx.sweep_series_submit(ts, scopes)
    assert code(gpu, lambda: ctx.set_series_sampling(False)) == -1
    r, _, _ = ctx.sweep_series_complete()
    assert same(r, want)
    ctx.set_series_sampling(False)
    ctx.invalidate_masks()
    r, _, _ = ctx.sweep_series(ts, scopes)
    assert ctx.series_sampled() == (0, 0) and not r["scalar"][:, 1:].view(np.uint64).any()
    # a slab pass on an armed context: -5
    ctx.set_series_sampling(True)
    contrib = torch.zeros(64, dtype=torch.float64, device="cuda"); gathered = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert code(gpu, lambda: ctx.series_dist_begin(ts, scopes, None, 0, 1, None, contrib, gathered, None)) == -5
    r, _, _ = ctx.sweep_series(ts, scopes)
    assert same(r, want)
    ctx.close()


@pytest.mark.parametrize("name,hooks,taken", [("random_2d_scalar_29x24x6", None, 4), ("moving_extremum_2d_21x21x9_aligned", None, 4),
                                              ("moving_extremum_3d_21x21x21x32", "one=0", 2), ("random_3d_scalar_13x12x11x4", None, 1)])
def test_armed_without_aux_arrays_is_the_unarmed_pass(gpu, name, hooks, taken, monkeypatch):
    """the one-launch pass (path 4) and the fused tail (path 2; one=0: a sparse series that the one-launch form would take) are taken as ever,
    nothing is launched for the switch"""
    if hooks:
        monkeypatch.setenv("FTKX_SERIES_HOOKS", hooks)
    g = load_golden(name)
    ts, scopes = steps_of(gpu, g)
    seen = []
    for arm in (False, True):
        ctx = make_context(gpu, g)
        if arm:
            ctx.set_series_sampling(True)
        paths, recs = [], []
        for _ in range(3):                        # (the first pass, the pass after a sparse one, and one more)
            ctx.invalidate_masks()
            recs.append(ctx.sweep_series(ts, scopes)[0]); paths.append(ctx.series_last_path()[0])
        ctx.sweep_series_submit(ts, scopes); ctx.sweep_series_submit(ts, scopes)
        for _ in range(2):
            recs.append(ctx.sweep_series_complete()[0]); paths.append(ctx.series_last_path()[0])
        assert ctx.series_sample_counts() == (0, 0, 0) and ctx.series_sampled() == (0, 0) and ctx.sample_counts() == (0, 0)
        seen.append((paths, recs))
        ctx.close()
    print(name, "paths", seen[0][0], seen[1][0])
    assert seen[0][0] == seen[1][0] and taken in seen[0][0], (seen[0][0], seen[1][0], taken)
    assert all(same(a, b) for a, b in zip(seen[0][1], seen[1][1]))


def test_never_armed_the_in_pass_kernel_is_never_launched(gpu):
    name = "random_3d_scalar_13x12x11x4"
    g = load_golden(name)
    B, Cf = fields(name)
    ts, scopes = steps_of(gpu, g)
    ctx = make_context(gpu, g)
    push_fields(ctx, g, B, Cf)                    # the arrays are there; the switch is not
    r0, _, _ = ctx.sweep_series(ts, scopes)
    for _ in range(3):
        ctx.invalidate_masks()
        ctx.sweep_series_submit(ts, scopes)
    for _ in range(3):
        r, _, _ = ctx.sweep_series_complete()
        assert same(r, r0) and not r["scalar"][:, 1:].view(np.uint64).any()
    assert ctx.series_sample_counts() == (0, 0, 0) and ctx.series_sampled() == (0, 0)
    ctx.close()


# ---- 7. trackers ------------------------------------------------------------------------------------------------------------------------------------
def tracked(gpu, g, names, extras, in_pass, deferred):
    tr = make_tracker(gpu, g, names)
    if in_pass:
        tr.set_sampling_in_pass(True)
    tr.initialize()
    if deferred:
        tr.set_deferred_collection(True, deferred)
    run_tracker_with(gpu, g, tr, extras)
    recs, o, ts = tr.get_critical_points()
    tr.finalize()
    curves, _ = tr.get_traced_critical_points()
    scal = tr.get_traced_scalars()
    tr.close()
    return recs, o, ts, curves, scal


@pytest.mark.parametrize("name", ["random_2d_scalar_29x24x6", "random_3d_scalar_13x12x11x4", "random_2d_vector_23x20x5"])
def test_trackers_sample_in_the_pass_deferred_or_not(gpu, name, monkeypatch):
    g = load_golden(name)
    B, Cf = fields(name)
    names = ["s", "b", "c"]
    extras = lambda k: [B[k], Cf[k]]      # noqa: E731
    base = tracked(gpu, g, names, extras, in_pass=False, deferred=0)      # the pass over finished records
    assert len(base[0]) == len(g["records"]) and base[0]["scalar"][:, 1].view(np.uint64).any() and base[0]["scalar"][:, 2].view(np.uint64).any()
    assert sum(len(c) for c in base[3]) > 0

    def check(got, what):
        assert same(got[0], base[0]) and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2]), (name, what)
        assert len(got[3]) == len(base[3]), (name, what)
        for c, d, s, u in zip(got[3], base[3], got[4], base[4]):
            assert np.array_equal(c, d) and SC.same_doubles(s, u), (name, what)

    check(tracked(gpu, g, names, extras, in_pass=True, deferred=0), "not deferred")
    check(tracked(gpu, g, names, extras, in_pass=True, deferred=1), "deferred, depth 1")
    check(tracked(gpu, g, names, extras, in_pass=True, deferred=3), "deferred, depth 3")
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,split=2")
    check(tracked(gpu, g, names, extras, in_pass=True, deferred=3), "deferred, depth 3, split")
    monkeypatch.delenv("FTKX_SERIES_HOOKS")
    # without the switch: deferred collection with components is refused as before
    tr = make_tracker(gpu, g, names)
    tr.initialize()
    tr.set_deferred_collection(True)
    push = tr.push_scalar_field_snapshot if g["nv"] == 1 else tr.push_vector_field_snapshot
    assert code(gpu, lambda: push(g["steps"][0], components=extras(0))) == -5
    tr.close()
