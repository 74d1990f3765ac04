"""The one-launch pass for small series (ftk_amd/csrc/one_kernel.hip, planned by series.hip: series_one_eligible / series_plan_one) ON its
limits, its edges and its ways out.  The series are those of tests/one_launch_cases.py; tests/test_one_launch_cases.py shows without a GPU
that each sits where it is said to sit (a workgroup's key store exactly full and one over, 8 192 and 8 193 blocks, 47 and 48 steps, 48
and 50 slices, 2^22 vertex-slices and more, blocks that straddle steps, the degenerate list exactly full, ...).

Every case runs on a fresh context -- the record count of an earlier pass and the passes a context sits out after a decline both change
eligibility -- and is compared with the CPU oracle's records stably sorted by tag, bit for bit and IN ORDER, with the factors; and with the
same series on a second context under FTKX_SERIES_HOOKS one=0 (the kernel chain), byte for byte, with the running resolution.  There are
no tolerances.  Every case asserts ftkx_series_last_path: "taken" is path 4 with none of the status bits 1 | 2 | 4 | 8, a decline is path 0
with the bit the case names, "not" is any other path without a decline -- a case that silently went another way fails.  Each case prints its
path, status, nblocks / nwg / bpw and the fullest workgroup's key count."""
import numpy as np
import pytest

import one_launch_cases as K
from common import assert_records_equal

pytestmark = pytest.mark.gpu

DECLINED = 1 | 2 | 4 | 8
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


@pytest.fixture(scope="module")
def cases(oracle):
    return K.cases()


def _ctx(gpu, c):
    ctx = gpu.Context(c.nd)
    ctx.set_mesh(c.dom, c.core, c.ext)
    o = dict(jacobian_symmetric=int(c.nv == 1), derive_jacobian=int(not c.given_j), tag_mode=c.tag_mode, compute_degrees=int(c.degrees))
    if c.bounds is not None:
        o["coords_bounds"] = c.bounds
    ctx.set_options(**o)
    return ctx


def _push(ctx, c, only=None):
    for t, a in c.slices().items():
        if only is not None and t not in only:
            continue
        if c.nv == 1:
            ctx.push_scalar_slice(t, a)
        else:
            ctx.push_slice(t, a, J=K.derived(c, a)[1] if c.given_j else None)


def _as_fixture(recs):
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = recs["aux"] & 1
    out["timestep"] = recs["aux"] >> 1
    return out


def _same(a, b):
    """record arrays identical byte for byte (NaN coordinates included)"""
    return len(a) == len(b) and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _assert_reference(recs, factors, c, what):
    """the records as they came, position by position (assert_records_equal alone would sort them first), and the factors"""
    ref, rf, _ = K.reference(c)
    assert [int(v) for v in factors] == rf, (what, list(factors), rf)
    assert len(recs) == len(ref), f"{what}: {len(recs)} records, expected {len(ref)}"
    bad = np.flatnonzero(recs["tag"] != ref["tag"])
    assert bad.size == 0, f"{what}: {bad.size} records out of tag order, the first at {int(bad[0])} of {len(ref)}"
    assert_records_equal(_as_fixture(recs), ref, coord_tol=0.0, what=what)


def _assert_path(c, path, status, what):
    if c.expect == "taken":
        assert path == 4 and not (status & DECLINED), f"{what}: path {path}, status {status}: the one-launch pass did not take it"
    elif c.expect == "not":
        assert path in (1, 2, 5) and not (status & DECLINED), f"{what}: path {path}, status {status}"
    else:
        assert path == 0 and (status & DECLINED) == c.expect, f"{what}: path {path}, status {status}: expected a decline with {c.expect}"


def _chain(gpu, c, monkeypatch):
    """the series on a context of its own under one=0 -> (records, factors, running resolution, path)"""
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0")
    ctx = _ctx(gpu, c)
    _push(ctx, c)
    want, wf, wrun = ctx.sweep_series(c.ts, c.scopes)
    path, status = ctx.series_last_path()
    ctx.close()
    monkeypatch.delenv("FTKX_SERIES_HOOKS")
    assert path != 4, (c.name, path, status)
    return want.copy(), wf.copy(), wrun, path


def _one(gpu, c, monkeypatch, keep=False):
    """the case under the default hooks on a fresh context, held to the oracle, to the kernel chain and to the way it says it goes
    -> (records, factors, running resolution[, the context])"""
    want, wf, wrun, wpath = _chain(gpu, c, monkeypatch)
    ctx = _ctx(gpu, c)
    _push(ctx, c)
    recs, f, run = ctx.sweep_series(c.ts, c.scopes)
    recs = recs.copy()
    path, status = ctx.series_last_path()
    p = c.plan()
    wg, _ = K.parked(c)
    print(c.name, "path", path, "status", status, "nblocks", p["nblocks"], "nwg", p["nwg"], "bpw", p["bpw"], "fullest workgroup", int(wg.max()) if len(wg) else 0,
          "records", len(recs), "the chain went", wpath)
    _assert_path(c, path, status, c.name)
    _assert_reference(recs, f, c, c.name)
    assert _same(recs, want) and np.array_equal(f, wf), f"{c.name}: {len(recs)} vs {len(want)} records of the kernel chain"
    assert run == wrun, (c.name, run, wrun)
    if keep:
        return recs, f, run, ctx
    ctx.close()
    return recs, f, run


# ---- limits ----------------------------------------------------------------------------------------------------------------------------

def test_key_store_exactly_full(gpu, cases, monkeypatch):
    """workgroup 85 parks exactly kOneKeys keys: taken"""
    recs, _, _ = _one(gpu, cases["keys_full"], monkeypatch)
    assert len(recs) == 1770


def test_key_store_one_over_then_sixteen_passes_sat_out(gpu, cases, monkeypatch):
    """workgroup 85 would park kOneKeys + 1 keys (the count the search reached: exactly one over): declined with SERIES_OVERFLOW, the
    records still those of the oracle.  The next 16 passes on that context go another way, the 17th is a one-launch pass again"""
    over, again = cases["keys_over"], cases["keys_over_again"]
    _, _, _, ctx = _one(gpu, over, monkeypatch, keep=True)
    for i in range(17):
        recs, f, _ = ctx.sweep_series(again.ts, again.scopes)
        path, status = ctx.series_last_path()
        print("pass", i + 1, "after the decline: path", path, "status", status)
        assert (path == 4) == (i == 16) and not (status & DECLINED), (i, path, status)
        if i in (0, 15, 16):
            _assert_reference(recs, f, again, f"pass {i + 1} after the decline")
    ctx.close()


@pytest.mark.parametrize("name", ["blocks_2d_at", "blocks_2d_over", "blocks_3d_at", "blocks_3d_over"])
def test_block_limit(gpu, cases, monkeypatch, name):
    _one(gpu, cases[name], monkeypatch)


@pytest.mark.parametrize("name", ["steps_47", "steps_48"])
def test_steps_and_slices(gpu, cases, monkeypatch, name):
    _one(gpu, cases[name], monkeypatch)


@pytest.mark.parametrize("name", ["gapped_24", "gapped_25"])
def test_steps_and_slices_with_gaps(gpu, cases, monkeypatch, name):
    """timesteps 0, 2, 4, ... of both scopes: two slices per step.  Held to the oracle and the kernel chain like every case, and to the
    host-driven batch (FTKX_SERIES=0)"""
    c = cases[name]
    recs, f, run = _one(gpu, c, monkeypatch)
    monkeypatch.setenv("FTKX_SERIES", "0")
    ctx = _ctx(gpu, c)
    _push(ctx, c)
    want, wf, wrun = ctx.sweep_series(c.ts, c.scopes)
    assert ctx.series_last_path()[0] == 0
    assert _same(recs, want) and np.array_equal(f, wf) and run == wrun, name
    ctx.close()


@pytest.mark.parametrize("name", ["vertices_at", "vertices_over"])
def test_vertex_rule(gpu, cases, monkeypatch, name):
    """2048 x 1024 x 2 slices = 2^22.  The factor, 8192, comes from a vertex far outside the core: the reduction reads the whole array"""
    _, f, _ = _one(gpu, cases[name], monkeypatch)
    assert set(int(v) for v in f) == {8192}


# ---- edges -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["straddle_2d", "straddle_3d", "no_record", "one_record"])
def test_blocks_that_straddle_steps_empty_blocks_short_last_block(gpu, cases, monkeypatch, name):
    recs, _, _ = _one(gpu, cases[name], monkeypatch)
    assert len(recs) == {"no_record": 0, "one_record": 1}.get(name, len(recs))


def _reclassified_by_the_chain(gpu, c, monkeypatch):
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0")
    ctx = _ctx(gpu, c)
    _push(ctx, c)
    ctx.sweep_series(c.ts, c.scopes)
    n = ctx.stats()["reclassified"]
    ctx.close()
    monkeypatch.delenv("FTKX_SERIES_HOOKS")
    return n


@pytest.mark.parametrize("name", ["plateau_2d", "plateau_3d"])
def test_degenerate_list_exactly_full(gpu, cases, monkeypatch, name):
    """every (corner, type) pair of the first block's rounds is degenerate: 384 (2D) / 960 (3D) entries, the size of the list.  3D: the
    records behind the plateau reach the fragile list; their types are the oracle's (held by every case) and as many were classified
    again on the host as in the kernel chain's pass"""
    c = cases[name]
    recs, _, _, ctx = _one(gpu, c, monkeypatch, keep=True)
    n = ctx.stats()["reclassified"]
    ctx.close()
    assert len(recs) > 0
    if c.nd == 3:
        m = _reclassified_by_the_chain(gpu, c, monkeypatch)
        print(name, "reclassified", n, "the chain", m)
        assert n > 0 and n == m, (n, m)


def test_fragile_list_too_small(gpu, cases, monkeypatch):
    """more fragile records than the list of a fresh context holds (4 096), no workgroup over its key store: declined with SERIES_OVERFLOW,
    the records still the oracle's; the list has grown, and a second sweep of the context gives the same records without a decline"""
    c = cases["fragile_over"]
    recs, f, run, ctx = _one(gpu, c, monkeypatch, keep=True)
    n = ctx.stats()["reclassified"]
    print("fragile records", n)
    assert n > 4096, n
    again, f2, run2 = ctx.sweep_series(c.ts, c.scopes)
    path, status = ctx.series_last_path()
    print("second sweep: path", path, "status", status, "reclassified", ctx.stats()["reclassified"])
    assert path != 0 and not (status & DECLINED), (path, status)
    assert _same(again, recs) and np.array_equal(f2, f) and run2 == run and ctx.stats()["reclassified"] == n
    ctx.close()


@pytest.mark.parametrize("name", ["ordinal_only", "interval_only", "mixed_scopes"])
def test_scopes(gpu, cases, monkeypatch, name):
    _one(gpu, cases[name], monkeypatch)


@pytest.mark.parametrize("name", ["image_bounds", "reference_tags", "work_index_tags", "degrees_2d", "vector_derived_j", "vector_given_j", "offset_mesh", "border_records"])
def test_other_ways_in(gpu, cases, monkeypatch, name):
    _one(gpu, cases[name], monkeypatch)


def test_a_component_exactly_at_the_cap_leaves_the_running_resolution_alone(gpu, cases, monkeypatch):
    """the smallest non-zero component is 1 / 256 = 1 / hint to the bit: only components BELOW it lower the running resolution"""
    _, f, run = _one(gpu, cases["at_the_cap"], monkeypatch)
    assert run == DBL_MAX and set(int(v) for v in f) == {256}, (run, f)


@pytest.mark.parametrize("name", ["inf", "ambiguous"])
def test_declines_the_kernel_raises(gpu, cases, monkeypatch, name):
    _one(gpu, cases[name], monkeypatch)


# ---- how callers drive it ------------------------------------------------------------------------------------------------------------------

def _whole(gpu, c, monkeypatch):
    recs, f, run, ctx = _one(gpu, c, monkeypatch, keep=True)
    return recs, f, run, ctx


def test_step_by_step_with_the_running_resolution_carried_by_the_caller(gpu, cases, monkeypatch):
    c = cases["reference_tags"]
    want, wf, wrun, ctx = _whole(gpu, c, monkeypatch)
    run, parts, fs = None, [], []
    for t, s in zip(c.ts, c.scopes):
        r, f, run = ctx.sweep_series([t], [s], running_resolution=run)
        assert ctx.series_last_path()[0] == 4, (t, ctx.series_last_path())
        parts.append(r.copy()); fs.append(int(f[0]))
    assert _same(np.concatenate(parts), want) and fs == [int(v) for v in wf] and run == wrun
    ctx.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_passes_in_flight(gpu, cases, monkeypatch, depth):
    c = cases["mixed_scopes"]
    want, wf, wrun, ctx = _whole(gpu, c, monkeypatch)
    for _ in range(depth):
        ctx.sweep_series_submit(c.ts, c.scopes)
    for i in range(depth):
        r, f, run = ctx.sweep_series_complete()
        assert ctx.series_last_path()[0] == 4, (i, ctx.series_last_path())
        assert _same(r, want) and np.array_equal(f, wf) and run == wrun, i
    ctx.close()


@pytest.mark.parametrize("first_is_one", [True, False])
def test_a_chained_second_half_of_the_other_form(gpu, cases, monkeypatch, first_is_one):
    """the second half continues ON THE DEVICE from the first's running minimum; one half is a one-launch pass, the other the kernel chain
    (the hook is read when a pass is planned)"""
    c = cases["reference_tags"]
    want, wf, wrun, ctx = _whole(gpu, c, monkeypatch)
    h = c.n // 2
    hooks = ["one=1", "one=0"] if first_is_one else ["one=0", "one=1"]
    monkeypatch.setenv("FTKX_SERIES_HOOKS", hooks[0])
    ctx.sweep_series_submit(c.ts[:h], c.scopes[:h])
    monkeypatch.setenv("FTKX_SERIES_HOOKS", hooks[1])
    ctx.sweep_series_submit(c.ts[h:], c.scopes[h:], chain=True)
    a, fa, _ = ctx.sweep_series_complete()
    a, pa = a.copy(), ctx.series_last_path()[0]
    b, fb, runb = ctx.sweep_series_complete()
    pb = ctx.series_last_path()[0]
    print("chained halves: paths", pa, pb)
    assert (pa == 4) == first_is_one and (pb == 4) == (not first_is_one) and pa != 0 and pb != 0, (pa, pb)
    assert _same(np.concatenate([a, b]), want) and np.array_equal(np.concatenate([fa, fb]), wf) and runb == wrun
    ctx.close()


def test_a_slice_dropped_and_pushed_again_between_passes(gpu, cases, monkeypatch):
    c = cases["mixed_scopes"]
    want, wf, wrun, ctx = _whole(gpu, c, monkeypatch)
    ctx.drop_slice(3)
    _push(ctx, c, only=[3])
    r, f, run = ctx.sweep_series(c.ts, c.scopes)
    assert ctx.series_last_path()[0] == 4
    assert _same(r, want) and np.array_equal(f, wf) and run == wrun
    ctx.close()
