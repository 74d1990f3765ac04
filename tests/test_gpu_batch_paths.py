"""The host-driven batch (ftkx_sweep_enqueue_many / ftkx_sweep_collect, csrc/collect.hip) where it leaves the straight road: a hit buffer
that is too small for the batch (regrown, the batch replayed), two quantisation factors in one batch (a slice's masks rebuilt in a second
sub-batch), both at once.  Small random series, every vertex near a critical point: the records are the oracle's (pyoracle.track on the
same arrays) and those of the same batch with the cull switched off (exact_only).  The plan behind all this is enumerated without a GPU
in tests/test_batch_plan_host.py."""
import numpy as np
import pytest

from common import assert_records_equal

pytestmark = pytest.mark.gpu

# name -> (nd, nv, dims, seed, records and factors as oracle/pyoracle.py::track finds them)
SERIES = {
    "regrow_2d": (2, 2, (128, 96), 7, 76000, [16384, 16384, 16384]),
    "regrow_3d": (3, 1, (24, 20, 18), 7, 71827, [16384, 16384, 16384]),
    "two_factors": (2, 2, (64, 48), 1, 17880, [16384, 65536, 65536]),
    "two_factors_regrow": (2, 2, (160, 128), 7, 127886, [16384, 65536, 65536]),
}
NT = 3
FIRST_CAPACITY = 1 << 16            # records the hit buffer holds before any batch has grown it (csrc/collect.hip)
_cache = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def _series(name):
    """the arrays (one generator per series, steps drawn in order), the oracle's records in tag order and its factors: computed once"""
    if name not in _cache:
        import pyoracle
        nd, nv, dims, seed, count, factors = SERIES[name]
        rng = np.random.default_rng(seed)
        shape = tuple(reversed(dims)) + ((nd,) if nv > 1 else ())
        steps = [rng.standard_normal(shape) for _ in range(NT)]
        ref, rf, _ = pyoracle.track(steps, nd, nv, tag_mode=pyoracle.TAG_EXACT64, nthreads=4)
        assert len(ref) == count and [int(f) for f in rf] == factors, (name, len(ref), rf)
        _cache[name] = (steps, ref[np.argsort(ref["tag"], kind="stable")], factors)
        for a in steps:
            a.setflags(write=False)
    return _cache[name]


def _ctx(gpu, name, **opts):
    nd, nv, dims = SERIES[name][:3]
    scalar = nv == 1
    dom = ([2 if scalar else 1] * nd, [d - (3 if scalar else 2) for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=int(scalar), derive_jacobian=1, tag_mode=gpu.TAG_EXACT64, **opts)
    for t, a in enumerate(_series(name)[0]):      # no slices_prepare, no slice_resolution: the slices' maxima stay unknown
        (ctx.push_scalar_slice if scalar else ctx.push_slice)(t, a)
    return ctx


def _scopes(gpu):
    return [gpu.SCOPE_BOTH if t + 1 < NT else gpu.SCOPE_ORDINAL for t in range(NT)]


def _batch(gpu, ctx, factors):
    ctx.sweep_enqueue_many(range(NT), _scopes(gpu), factors)
    return np.array(ctx.sweep_collect())


def _as_fixture(recs):
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = recs["aux"] & 1
    out["timestep"] = recs["aux"] >> 1
    return out


def _exact_only(gpu, name):
    """the same batch with every simplex tested (no masks, no cull, no survivor lists): records and statistics, computed once"""
    key = (name, "exact_only")
    if key not in _cache:
        ctx = _ctx(gpu, name, exact_only=1)
        recs = _batch(gpu, ctx, _series(name)[2])
        _cache[key] = (recs, ctx.stats())
        ctx.close()
    return _cache[key]


def _check(gpu, name, got, what):
    steps, ref, factors = _series(name)
    assert np.array_equal(got["tag"], np.sort(got["tag"])), what + ": records not in tag order"
    assert_records_equal(_as_fixture(got), ref, coord_tol=0.0, what=what)      # tags, types, (ordinal, timestep) exact; x, t, scalar bit for bit
    assert got.tobytes() == _exact_only(gpu, name)[0].tobytes(), what + ": not the records of exact_only"


def _mask_launches(ctx):
    return ctx.kernel_times()["mask_kernel"][1]


@pytest.mark.parametrize("name", ["regrow_2d", "regrow_3d"])
def test_hit_buffer_regrown(gpu, name):
    """more records than the hit buffer's first capacity (the survivor lists, 2^20 entries, do not overflow): the first collect counts,
    grows the buffer and replays the batch -- the replay finds the masks the first attempt built and committed, so no mask launch is
    among the kernels of the attempt that counted; the second collect of the same context finds room: one attempt, the same records"""
    steps, ref, factors = _series(name)
    assert len(ref) > FIRST_CAPACITY
    ctx = _ctx(gpu, name)
    ctx.set_profiling(1)
    first = _batch(gpu, ctx, factors)
    st = ctx.stats()
    assert _mask_launches(ctx) == 0, "the attempt that fitted was the first: the hit buffer was not regrown"
    _check(gpu, name, first, name + " first collect")
    assert st["hits"] == len(ref)
    if SERIES[name][0] == 3:
        assert st["reclassified"] == _exact_only(gpu, name)[1]["reclassified"]
    ctx.invalidate_masks()                                     # so that an attempt that runs to the end shows as one mask launch
    second = _batch(gpu, ctx, factors)
    assert _mask_launches(ctx) == 1, "the second collect regrew a buffer"
    assert second.tobytes() == first.tobytes()
    assert ctx.stats() == st
    ctx.close()


@pytest.mark.parametrize("name", ["two_factors", "two_factors_regrow"])
def test_two_factors_in_one_batch(gpu, name):
    """[16384, 65536, 65536] over slices whose maxima the context does not know: slice 1 gets masks under 16384 for the first step and
    again, in a second sub-batch, under 65536 (tests/test_batch_plan_host.py: exactly two) -- the records are those of the same steps
    swept one ftkx_sweep at a time on a second context, byte for byte.  The larger series also overflows the hit buffer: the replay
    goes through the counter reset between the sub-batches a second time."""
    steps, ref, factors = _series(name)
    assert len(set(factors)) == 2 and (len(ref) > FIRST_CAPACITY) == (name == "two_factors_regrow")
    ctx = _ctx(gpu, name)
    ctx.set_profiling(1)
    got = _batch(gpu, ctx, factors)
    # the attempt that counted: without a regrowth two mask launches (two sub-batches); in the replay slice 1 is rebuilt under each factor again
    assert _mask_launches(ctx) == 2
    _check(gpu, name, got, name)
    one = _ctx(gpu, name)
    parts = [np.array(one.sweep(t, s, f)) for t, s, f in zip(range(NT), _scopes(gpu), factors)]
    each = np.concatenate(parts)
    assert each[np.argsort(each["tag"], kind="stable")].tobytes() == got.tobytes()
    again = _batch(gpu, ctx, factors)                          # the same context once more: masks as the batch left them
    assert again.tobytes() == got.tobytes()
    for c in (ctx, one):
        c.close()
