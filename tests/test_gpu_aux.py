"""Auxiliary scalar fields sampled at critical points, on the GPU: ftkx_push_aux_slice / ftkx_sample_aux through Context and the trackers.
Sampling a fixture's own S gives scalar[0] back in slots 1 and 2 whichever way the records were swept; foreign fields give what the pinned
oracle gives with them as S -- from host FP64, float32 and lent device arrays alike; the kernel equals the host build of sample_steps.hpp;
the contract's error paths leave the records untouched; the trackers carry the slots into points, trajectories and files.
All comparisons of doubles are on bit patterns (a NaN equal to any NaN)."""
import re

import numpy as np
import pytest

import sample_cases as SC
from common import load_golden

pytestmark = pytest.mark.gpu

PATHS = ("series", "batch", "exact_only")
THREE_PATHS = ("random_2d_scalar_29x24x6", "random_3d_scalar_13x12x11x4")


def widest(name):
    """the largest spatial size in a fixture's name (..._WxHxT... / ..._WxHxDxT...)"""
    return max(int(v) for v in re.search(r"_(\d+(?:x\d+)+)", name).group(1).split("x")[:-1])


SMALL = [n for n in SC.scalar_golden_names() if widest(n) <= 32]
SELF_CASES = [(n, "series") for n in SMALL] + [(n, p) for n in THREE_PATHS for p in PATHS[1:]]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def make_context(gpu, g, tag_mode=None, exact_only=False, t0=0):
    """the fixture's steps resident in a context of the fixture's mesh and options (physical coordinates left out: no scalar depends on them)"""
    nd, scalar = g["nd"], g["nv"] == 1
    dom = SC.domain_of(g)
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(g["dims"])))
    kw = dict(jacobian_symmetric=scalar, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE if tag_mode is None else tag_mode, robust=int(g["robust"]), exact_only=int(exact_only))
    if g["type_filter"] is not None:
        kw.update(use_type_filter=1, type_filter=g["type_filter"])
    if g["degrees"]:
        kw["compute_degrees"] = 1
    ctx.set_options(**kw)
    for k, a in enumerate(g["steps"]):
        (ctx.push_scalar_slice if scalar else ctx.push_slice)(t0 + k, a)
    return ctx


def sweep_all(gpu, ctx, g, path="series", t0=0):
    DT = g["DT"]
    ts = np.arange(t0, t0 + DT, dtype=np.int32)
    scopes = np.array([gpu.SCOPE_BOTH] * (DT - 1) + [gpu.SCOPE_ORDINAL], dtype=np.int32)
    if path == "batch":
        ctx.sweep_enqueue_many(ts, scopes, [int(f) for f in g["factors"]])
        return ctx.sweep_collect()
    return ctx.sweep_series(ts, scopes)[0]


def sweep_by_scope(gpu, ctx, g):
    """every (step, scope) on its own: what FTKX_TAG_WORK_INDEX tags count inside"""
    out = []
    for t in range(g["DT"]):
        out.append(ctx.sweep(t, gpu.SCOPE_ORDINAL, int(g["factors"][t])))
        if t + 1 < g["DT"]:
            out.append(ctx.sweep(t, gpu.SCOPE_INTERVAL, int(g["factors"][t])))
    return np.concatenate(out)


def only_slots_changed(after, before):
    """every byte of every record but scalar[1] and scalar[2] is what it was, and those were zero"""
    assert not before["scalar"][:, 1:].view(np.uint64).any()
    a = after.copy()
    a["scalar"][:, 1:] = 0.0
    return a.tobytes() == before.tobytes()


def push_fields(ctx, g, B=None, Cf=None, t0=0):
    for t in range(g["DT"]):
        if B is not None:
            ctx.push_aux_slice(t0 + t, 1, B[t])
        if Cf is not None:
            ctx.push_aux_slice(t0 + t, 2, Cf[t])


# ---- 1. self-sampling ---------------------------------------------------------------------------------------------------------------------------
def test_small_fixtures_are_the_ones_named():
    for want in ("moving_extremum_3d_21x21x21x4_overflow", "moving_extremum_2d_21x21x9_aligned", "adversarial_3d_scalar_9x9x9x4", "huge_nan_3d_scalar_10x9x9x3",
                 "random_3d_scalar_13x12x11x4_norobust", "moving_extremum_3d_32x32x32x8_dyadic") + THREE_PATHS:
        assert want in SMALL
    assert "woven_128x128x10" not in SMALL and "singular_terraces_44x40x36x5" not in SMALL


@pytest.mark.parametrize("name,path", SELF_CASES)
def test_own_scalar_field_comes_back_in_slots_1_and_2(gpu, name, path):
    g = load_golden(name)
    ctx = make_context(gpu, g, exact_only=(path == "exact_only"))
    recs = sweep_all(gpu, ctx, g, path)
    assert len(recs) == len(g["records"])
    before = recs.copy()
    push_fields(ctx, g, g["steps"], g["steps"])
    assert ctx.sample_aux(recs) is recs
    assert ctx.sample_counts() == (1, len(recs))
    assert only_slots_changed(recs, before)
    assert SC.same_doubles(recs["scalar"][:, 1], before["scalar"][:, 0]), int((recs["scalar"][:, 1].copy().view(np.uint64) != before["scalar"][:, 0].copy().view(np.uint64)).sum())
    assert SC.same_doubles(recs["scalar"][:, 2], before["scalar"][:, 0])
    # ... which is the reference's own scalar[0]
    ref = g["records"][np.argsort(g["records"]["tag"], kind="stable")]
    got = recs[np.argsort(recs["tag"], kind="stable")]
    assert np.array_equal(got["tag"], ref["tag"]) and SC.same_doubles(got["scalar"][:, 1], ref["scalar"])
    ctx.close()


# ---- 2. foreign fields --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def foreign(gpu, oracle):
    """per case: the fixture, its records as the device-driven pass gives them, B and C per timestep and what the oracle makes of them"""
    out = {}

    def get(name):
        if name not in out:
            g = load_golden(name)
            ctx = make_context(gpu, g)
            recs = sweep_all(gpu, ctx, g)
            ctx.close()
            B = [SC.foreign_field(name, t, 0) for t in range(g["DT"])]
            Cf = [SC.foreign_field(name, t, 1) for t in range(g["DT"])]
            assert len(recs) >= 20 and (recs["aux"] & 1).any() and not (recs["aux"] & 1).all()
            e1 = SC.expected_for(recs["tag"], SC.foreign_expectation(oracle, name, 0))
            e2 = SC.expected_for(recs["tag"], SC.foreign_expectation(oracle, name, 1))
            recs.setflags(write=False)
            out[name] = (g, recs, B, Cf, e1, e2)
        return out[name]
    return get


@pytest.mark.parametrize("name", SC.FOREIGN)
def test_foreign_fields_against_the_oracle(gpu, foreign, name):
    g, recs0, B, Cf, e1, e2 = foreign(name)
    ctx = make_context(gpu, g)
    recs = recs0.copy()
    push_fields(ctx, g, B, Cf)
    ctx.sample_aux(recs)
    assert only_slots_changed(recs, recs0)
    assert SC.same_doubles(recs["scalar"][:, 1], e1), int((recs["scalar"][:, 1].copy().view(np.uint64) != e1.view(np.uint64)).sum())
    assert SC.same_doubles(recs["scalar"][:, 2], e2)
    # one slot alone: the other stays zero
    for t in range(g["DT"]):
        ctx.drop_slice(t)
    ctx2 = make_context(gpu, g)
    push_fields(ctx2, g, None, Cf)
    r2 = ctx2.sample_aux(recs0.copy())
    assert SC.same_doubles(r2["scalar"][:, 2], e2) and not r2["scalar"][:, 1].view(np.uint64).any()
    ctx.close(); ctx2.close()


@pytest.mark.parametrize("name", SC.FOREIGN)
def test_float32_field_is_the_push_of_the_widened_array(gpu, foreign, name):
    g, recs0, B, Cf, e1, e2 = foreign(name)
    with np.errstate(over="ignore"):
        B32 = [b.astype(np.float32) for b in B]                  # (1e300 becomes inf, 5e-324 becomes 0: both are values like any other)
    ctx = make_context(gpu, g)
    push_fields(ctx, g, [b.astype(np.float64) for b in B32], Cf)
    wide = ctx.sample_aux(recs0.copy())
    w0 = ctx.f32_counts()[0]
    push_fields(ctx, g, B32, None)
    assert ctx.f32_counts()[0] == w0 + g["DT"]                   # through the widen kernel
    narrow = ctx.sample_aux(recs0.copy())
    assert SC.same_doubles(narrow["scalar"][:, 1], wide["scalar"][:, 1]) and SC.same_doubles(narrow["scalar"][:, 2], e2)
    assert only_slots_changed(narrow, recs0)
    assert not SC.same_doubles(wide["scalar"][:, 1], e1)         # (the floats are not the doubles)
    ctx.close()


@pytest.mark.parametrize("name", SC.FOREIGN)
def test_lent_device_field_is_read_in_place_and_left_alone(gpu, foreign, name):
    import torch
    g, recs0, B, Cf, e1, e2 = foreign(name)
    ctx = make_context(gpu, g)
    alloc0 = ctx.array_counts()[0][0]
    Bd = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in B]
    Cd = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in Cf]
    keep = [t.clone() for t in Bd + Cd]
    torch.cuda.synchronize()
    for t in range(g["DT"]):
        ctx.push_aux_slice(t, 1, Bd[t], on_device=1)
        ctx.push_aux_slice(t, 2, Cd[t], on_device=1)
    assert ctx.array_counts()[0][0] == alloc0                    # lent: nothing allocated
    recs = ctx.sample_aux(recs0.copy())
    assert SC.same_doubles(recs["scalar"][:, 1], e1) and SC.same_doubles(recs["scalar"][:, 2], e2)
    for t in range(g["DT"]):
        ctx.drop_slice(t)
    ctx.close()
    torch.cuda.synchronize()
    for a, b in zip(Bd + Cd, keep):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))      # the caller's tensors: unchanged, and still the caller's


# ---- 3. device against host -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["work_index", "reference", "exact64"])
@pytest.mark.parametrize("name", SC.FOREIGN)
def test_kernel_equals_the_host_build_of_the_steps(gpu, name, mode):
    g = load_golden(name)
    tag_mode = {"work_index": gpu.TAG_WORK_INDEX, "reference": gpu.TAG_REFERENCE, "exact64": gpu.TAG_EXACT64}[mode]
    ctx = make_context(gpu, g, tag_mode=tag_mode)
    recs = sweep_by_scope(gpu, ctx, g) if mode == "work_index" else sweep_all(gpu, ctx, g)
    assert len(recs) == len(g["records"])
    B = [SC.foreign_field(name, t, 0) for t in range(g["DT"])]
    Cf = [SC.foreign_field(name, t, 1) for t in range(g["DT"])]
    push_fields(ctx, g, B, Cf)
    got = ctx.sample_aux(recs.copy())
    h1, h2, ok, bad = SC.host_sample(g, tag_mode, recs["tag"], recs["aux"], A1=B, A2=Cf)
    assert bad == 0 and ok.all()
    assert SC.same_doubles(got["scalar"][:, 1], h1) and SC.same_doubles(got["scalar"][:, 2], h2)
    ctx.close()


def test_wrapped_series_exact64_samples_reference_is_refused(gpu):
    name = "wrap_3d_scalar_16x15x14x3_t2000000"
    g = load_golden(name)
    t0 = g["t0"]
    ctx = make_context(gpu, g, tag_mode=gpu.TAG_EXACT64, t0=t0)
    recs = sweep_all(gpu, ctx, g, t0=t0)
    assert len(recs) == len(g["records"]) and int((recs["aux"] >> 1).min()) == t0
    push_fields(ctx, g, g["steps"], None, t0=t0)
    got = ctx.sample_aux(recs.copy())
    assert SC.same_doubles(got["scalar"][:, 1], recs["scalar"][:, 0])
    h1, _, ok, bad = SC.host_sample(g, SC.TAG_EXACT64, recs["tag"], recs["aux"], A1=g["steps"], t0=t0)
    assert bad == 0 and SC.same_doubles(got["scalar"][:, 1], h1)
    ctx.close()
    ctx = make_context(gpu, g, tag_mode=gpu.TAG_REFERENCE, t0=t0)
    recs = sweep_all(gpu, ctx, g, t0=t0)
    push_fields(ctx, g, g["steps"], None, t0=t0)
    before = recs.copy()
    with pytest.raises(gpu.FtkxError) as e:
        ctx.sample_aux(recs)
    assert e.value.code == -5 and recs.tobytes() == before.tobytes()
    ctx.close()


# ---- 4. contract ----------------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    name = "random_2d_scalar_29x24x6"
    g = load_golden(name)
    ctx = make_context(gpu, g)
    recs = sweep_all(gpu, ctx, g)
    before = recs.copy()
    DT = g["DT"]
    B = [SC.foreign_field(name, t, 0) for t in range(DT)]
    # no slot resident: OK, nothing done; n == 0: OK
    assert ctx.sample_aux(recs).tobytes() == before.tobytes() and ctx.sample_counts() == (0, 0)
    assert len(ctx.sample_aux(np.zeros(0, dtype=gpu.CP_DTYPE))) == 0
    # slots 0 and 3, a wrong extent
    for slot in (0, 3):
        with pytest.raises(gpu.FtkxError) as e:
            ctx.push_aux_slice(0, slot, B[0])
        assert e.value.code == -1
    for wrong in (B[0][:-1], B[0].reshape(-1)[:17], np.zeros((25, 29))):
        with pytest.raises(gpu.FtkxError) as e:
            ctx.push_aux_slice(0, 1, wrong)
        assert e.value.code == -1
    # an aux array missing at the last timestep, which interval records of the step before it read
    counts0 = ctx.array_counts()
    for t in range(DT - 1):
        ctx.push_aux_slice(t, 1, B[t])
    assert (recs["aux"] >> 1).max() == DT - 1
    with pytest.raises(gpu.FtkxError) as e:
        ctx.sample_aux(recs)
    assert e.value.code == -4 and recs.tobytes() == before.tobytes() and ctx.sample_counts() == (0, 0)
    # ... but the records of the steps whose arrays are all there are sampled
    part = recs[(recs["aux"] >> 1) + 1 - (recs["aux"] & 1) <= DT - 2].copy()
    assert 0 < len(part) < len(recs)
    ctx.sample_aux(part)
    assert ctx.sample_counts() == (1, len(part)) and part["scalar"][:, 1].view(np.uint64).any()
    # a field slice that is not resident
    ctx.push_aux_slice(DT - 1, 1, B[DT - 1])
    ctx.drop_slice(DT - 1)                                      # takes its aux array along
    with pytest.raises(gpu.FtkxError) as e:
        ctx.sample_aux(recs)
    assert e.value.code == -4 and recs.tobytes() == before.tobytes()
    # after drop_slice the arrays are back in the pool: nothing is held by a slice, nothing leaked
    for t in range(DT - 1):
        ctx.drop_slice(t)
    alloc, pooled = ctx.array_counts()
    assert alloc[0] == counts0[0][0] + DT and pooled[0] == min(12, alloc[0])
    # pushed again, the arrays come out of the pool
    for k, a in enumerate(g["steps"]):
        ctx.push_scalar_slice(k, a)
        ctx.push_aux_slice(k, 2, B[k])
    assert ctx.array_counts()[0][0] == alloc[0]
    got = ctx.sample_aux(recs.copy())
    h, _, _, bad = SC.host_sample(g, SC.TAG_REFERENCE, recs["tag"], recs["aux"], A1=B)
    assert bad == 0 and SC.same_doubles(got["scalar"][:, 2], h) and not got["scalar"][:, 1].view(np.uint64).any()
    # a record of another mesh is refused, nothing is written
    bad_recs = recs.copy(); bad_recs["tag"][5] = np.uint64(2 ** 62)
    snapshot = bad_recs.copy()
    with pytest.raises(gpu.FtkxError) as e:
        ctx.sample_aux(bad_recs)
    assert e.value.code == -1 and bad_recs.tobytes() == snapshot.tobytes()
    ctx.close()


def test_relaunch_times_the_kernel_and_writes_nothing(gpu):
    name = "random_3d_scalar_13x12x11x4"
    g = load_golden(name)
    ctx = make_context(gpu, g)
    recs = sweep_all(gpu, ctx, g)
    push_fields(ctx, g, g["steps"], None)
    before = recs.copy()
    ms = ctx.debug_sample_relaunch(recs, 3)
    assert len(ms) == 3 and all(0.0 < m < 50.0 for m in ms) and recs.tobytes() == before.tobytes() and ctx.sample_counts() == (0, 0)
    ctx.close()


# ---- 5. trackers ----------------------------------------------------------------------------------------------------------------------------------
def make_tracker(gpu, g, names, streaming=False):
    nd, nv, D = g["nd"], g["nv"], g["dims"]
    tr = (gpu.CriticalPointTracker2DRegular if nd == 2 else gpu.CriticalPointTracker3DRegular)()
    if nv == 1:
        tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
        tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
    else:
        tr.set_scalar_field_source(gpu.SOURCE_NONE); tr.set_vector_field_source(gpu.SOURCE_GIVEN)
        tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(False)
    tr.set_domain(*SC.domain_of(g))
    tr.set_array_domain([0] * nd, D)
    tr.set_enable_robust_detection(g["robust"])
    if streaming:
        tr.set_enable_streaming_trajectories(True)
    if names is not None:
        tr.set_scalar_components(names)
    return tr


def run_tracker_with(gpu, g, tr, extras):
    """extras(k) -> the components of snapshot k"""
    push = tr.push_scalar_field_snapshot if g["nv"] == 1 else tr.push_vector_field_snapshot
    for k, a in enumerate(g["steps"]):
        push(a, components=extras(k))
        if k:
            tr.advance_timestep()
        if k == g["DT"] - 1:
            tr.update_timestep()


@pytest.mark.parametrize("name", THREE_PATHS)
def test_trackers_carry_the_components(gpu, foreign, tmp_path, name):
    g, recs0, B, Cf, e1, e2 = foreign(name)
    by_tag = {int(t): (a, b) for t, a, b in zip(recs0["tag"], e1, e2)}
    names = ["s", "b", "c"]
    tr = make_tracker(gpu, g, names)
    tr.initialize()
    run_tracker_with(gpu, g, tr, lambda k: [B[k], Cf[k]])
    recs, o, ts = tr.get_critical_points()
    assert len(recs) == len(recs0)
    exp = np.array([by_tag[int(t)] for t in recs["tag"]])
    assert SC.same_doubles(recs["scalar"][:, 1], exp[:, 0]) and SC.same_doubles(recs["scalar"][:, 2], exp[:, 1])
    s0 = dict(zip(recs0["tag"].tolist(), recs0["scalar"][:, 0]))
    assert SC.same_doubles(recs["scalar"][:, 0], np.array([s0[int(t)] for t in recs["tag"]]))
    # the text writer prints the names: byte-identical to the free function on the same records
    recs["aux"] = (ts.astype(np.uint32) << 1) | (o.astype(np.uint32) & 1)
    p1, p2 = tmp_path / "tracker.txt", tmp_path / "free.txt"
    tr.write_critical_points_text(p1)
    gpu.write_critical_points(p2, recs, scalar_names=names)
    txt = open(p1, "rb").read()
    assert txt == open(p2, "rb").read() and b"b=" in txt and b"c=" in txt
    # traced trajectories carry them
    tr.finalize()
    curves, _ = tr.get_traced_critical_points()
    scal = tr.get_traced_scalars()
    assert sum(len(c) for c in curves) > 0
    for c, s in zip(curves, scal):
        e = np.array([by_tag[int(t)] for t in c]).reshape(-1, 2)
        assert SC.same_doubles(s[:, 1], e[:, 0]) and SC.same_doubles(s[:, 2], e[:, 1])
    tr.close()
    # ... and so do streaming trajectories
    tr = make_tracker(gpu, g, names, streaming=True)
    tr.set_tag_mode(gpu.TAG_EXACT64)
    tr.initialize()
    run_tracker_with(gpu, g, tr, lambda k: [B[k], Cf[k]])
    tr.finalize()
    curves, _ = tr.get_traced_critical_points()
    scal = tr.get_traced_scalars()
    assert sum(len(c) for c in curves) > 0
    for c, s in zip(curves, scal):
        e = np.array([by_tag[int(t)] for t in c]).reshape(-1, 2)
        assert SC.same_doubles(s[:, 1], e[:, 0]) and SC.same_doubles(s[:, 2], e[:, 1])
    tr.close()


def test_vector_tracker_with_two_components(gpu, foreign):
    name = "random_2d_vector_23x20x5"
    g, recs0, B, Cf, e1, e2 = foreign(name)
    by_tag = dict(zip(recs0["tag"].tolist(), e1))
    tr = make_tracker(gpu, g, ["none", "b"])
    tr.initialize()
    run_tracker_with(gpu, g, tr, lambda k: [B[k]])
    recs, _, _ = tr.get_critical_points()
    assert len(recs) == len(recs0) and not recs["scalar"][:, 0].view(np.uint64).any() and not recs["scalar"][:, 2].view(np.uint64).any()
    assert SC.same_doubles(recs["scalar"][:, 1], np.array([by_tag[int(t)] for t in recs["tag"]]))
    tr.close()


def test_tracker_without_components_is_what_it_was(gpu):
    g = load_golden("random_2d_scalar_29x24x6")
    tr = make_tracker(gpu, g, None)
    tr.initialize()
    run_tracker_with(gpu, g, tr, lambda k: None)
    recs, _, _ = tr.get_critical_points()
    assert len(recs) == len(g["records"]) and not recs["scalar"][:, 1:].view(np.uint64).any()
    tr.close()


def test_unsupported_combinations_and_wrong_counts(gpu):
    g = load_golden("random_2d_scalar_29x24x6")
    B = SC.foreign_field("random_2d_scalar_29x24x6", 0, 0)
    S = g["steps"][0]

    def code(f):
        with pytest.raises(gpu.FtkxError) as e:
            f()
        return e.value.code

    # temporal smoothing, several devices, slab mode: at initialize()
    tr = make_tracker(gpu, g, ["s", "b"]); tr.set_temporal_smoothing(1.0, 3)
    assert code(tr.initialize) == -5
    tr.close()
    tr = gpu.CriticalPointTracker2DRegular(device_ids=[0, 0])
    tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
    tr.set_domain(*SC.domain_of(g)); tr.set_array_domain([0, 0], g["dims"]); tr.set_scalar_components(["s", "b"])
    assert code(tr.initialize) == -5
    tr.close()
    from ftk_amd import _lib
    hub = _lib.load().ftkx_slab_hub_create(2)
    tr = make_tracker(gpu, g, ["s", "b"]); tr.initialize(); tr.set_slab_hub(hub, 0, 12)
    assert code(lambda: tr.push_scalar_field_snapshot(S, components=[B])) == -5
    assert code(tr.initialize) == -5
    tr.close()
    _lib.load().ftkx_slab_hub_destroy(hub)
    # deferred collection: at the push
    tr = make_tracker(gpu, g, ["s", "b"]); tr.initialize(); tr.set_deferred_collection(True)
    assert code(lambda: tr.push_scalar_field_snapshot(S, components=[B])) == -5
    tr.close()
    # the number of extras is the number of names minus one, with every push; names: one to three
    tr = make_tracker(gpu, g, ["s", "b", "c"]); tr.initialize()
    assert code(lambda: tr.push_scalar_field_snapshot(S, components=[B])) == -1
    assert code(lambda: tr.push_scalar_field_snapshot(S)) == -1
    assert code(lambda: tr.set_scalar_components([])) == -1 and code(lambda: tr.set_scalar_components(["a", "b", "c", "d"])) == -1
    tr.close()
    tr = make_tracker(gpu, g, None); tr.initialize()
    assert code(lambda: tr.push_scalar_field_snapshot(S, components=[B])) == -1
    tr.close()
