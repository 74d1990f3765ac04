"""Spatial Gaussian smoothing on the GPU (ftk_amd/csrc/conv_kernels.hip): ftkx_conv2D / ftkx_conv3D against the reference's own outputs
(tests/golden/conv/) and, on either side of every tile edge and for all five kernel sizes, against the numpy restatement of
tests/conv_cases.py -- as uint64; then ftkx_set_spatial_smoothing through the push, the series pass and the tracker: a context that smooths
raw slices must give what a context gives that is handed the reference's smoothed slices."""
import numpy as np
import pytest

import conv_cases as CC
from common import assert_records_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


@pytest.fixture(scope="module")
def ctx2(gpu):
    c = gpu.Context(2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx3(gpu):
    c = gpu.Context(3)
    yield c
    c.close()


def device_conv(ctx, a, w):
    """a: numpy array, x last; -> what ftkx_conv2D / 3D writes, on the host.  The output starts as a pattern no convolution gives."""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    keep = src.clone()
    out = torch.full(a.shape, 777.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dims = list(reversed(a.shape))
    if a.ndim == 2:
        ctx.conv2D(src.data_ptr(), dims[0], dims[1], w, w.shape[0], out.data_ptr())
    else:
        ctx.conv3D(src.data_ptr(), dims[0], dims[1], dims[2], w, w.shape[0], out.data_ptr())
    assert torch.equal(src.view(torch.int64), keep.view(torch.int64)), "the input was written"
    return out.cpu().numpy()


@pytest.mark.parametrize("name", CC.fixture_names())
def test_fixtures(gpu, ctx2, ctx3, name):
    f = CC.load(name)
    got = device_conv(ctx2 if int(f["nd"]) == 2 else ctx3, f["input"], f["weights"])
    assert np.array_equal(got.view(np.uint64), f["output"].view(np.uint64)), name


def test_series_fixture(gpu, ctx2):
    s = CC.series()
    for k in range(int(s["DT"])):
        assert np.array_equal(device_conv(ctx2, s["raw"][k], s["weights"]).view(np.uint64), s["smoothed"][k].view(np.uint64)), k


@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_border_shapes_2d(gpu, ctx2, ksize):
    w = gpu.gaussian_kernel(2, 0.75 + 0.25 * ksize, ksize)
    seen = set()
    for shape in CC.SHAPES_2D:
        a = CC.shape_input(shape, ksize)
        seen |= {"inf"} if np.isinf(a).any() else ({"nan"} if np.isnan(a).any() else set())
        assert CC.same_bits(device_conv(ctx2, a, w), CC.conv(a, w)), (shape, ksize)
    assert seen == {"inf", "nan"}


@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_border_shapes_3d(gpu, ctx3, ksize):
    w = gpu.gaussian_kernel(3, 0.75 + 0.25 * ksize, ksize)
    seen = set()
    for shape in CC.SHAPES_3D:
        a = CC.shape_input(shape, ksize)
        seen |= {"inf"} if np.isinf(a).any() else ({"nan"} if np.isnan(a).any() else set())
        assert CC.same_bits(device_conv(ctx3, a, w), CC.conv(a, w)), (shape, ksize)
    assert seen == {"inf", "nan"}


def test_conv_argument_errors(gpu, ctx2, ctx3):
    import torch
    a = torch.zeros(64, dtype=torch.float64, device="cuda"); b = torch.zeros(64, dtype=torch.float64, device="cuda")
    w = np.full(81, 1.0 / 81)
    L = ctx2._L
    E = gpu._lib.E_INVALID
    assert L.ftkx_conv2D(ctx2._h, a.data_ptr(), 8, 8, w.ctypes.data, 4, b.data_ptr()) == E
    assert L.ftkx_conv2D(ctx2._h, a.data_ptr(), 8, 8, w.ctypes.data, 11, b.data_ptr()) == E
    assert L.ftkx_conv2D(ctx2._h, a.data_ptr(), 0, 8, w.ctypes.data, 3, b.data_ptr()) == E
    assert L.ftkx_conv2D(ctx2._h, a.data_ptr(), 8, 8, None, 3, b.data_ptr()) == E
    assert L.ftkx_conv2D(ctx2._h, a.data_ptr(), 8, 8, w.ctypes.data, 3, a.data_ptr()) == E                   # in place
    assert L.ftkx_conv2D(ctx2._h, a.data_ptr(), 8, 4, w.ctypes.data, 3, a.data_ptr() + 8 * 16) == E          # overlapping
    assert L.ftkx_conv3D(ctx3._h, a.data_ptr(), 4, 4, 4, w.ctypes.data, 2, b.data_ptr()) == E
    assert L.ftkx_set_spatial_smoothing(ctx2._h, 1.0, 4) == E and L.ftkx_set_spatial_smoothing(ctx2._h, -1.0, 3) == E
    assert L.ftkx_set_spatial_smoothing(ctx2._h, 0.0, 0) == 0


# ---- the push path -------------------------------------------------------------------------------------------------------------------------
def scalar_context(gpu, dims):
    nd = len(dims)
    dom = ([2] * nd, [d - 3 for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
    return ctx


def as_fixture(recs):
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = recs["aux"] & 1
    out["timestep"] = recs["aux"] >> 1
    return out


def series_of(gpu, ctx, slices, on_device=0):
    """pushes the slices (on_device 1 / 2: as device tensors, checked to be unchanged afterwards) and sweeps every step in one pass"""
    import torch
    nt = len(slices)
    tensors = []
    for t, a in enumerate(slices):
        if on_device:
            x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            torch.cuda.synchronize()
            tensors.append((x, x.clone()))
            ctx.push_scalar_slice(t, x, on_device=on_device)
        else:
            ctx.push_scalar_slice(t, a)
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    recs, factors, _ = ctx.sweep_series(range(nt), scopes)
    for x, before in tensors:
        assert torch.equal(x.view(torch.int64), before.view(torch.int64)), "a pushed tensor was written"
    return recs, [int(f) for f in factors]


def same_records(a, b):
    return len(a) == len(b) and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def woven(gpu, oracle):
    """the noisy woven series: what a context without smoothing gives for the reference's smoothed slices and for the raw ones, and the
    oracle on the smoothed slices -- computed once"""
    s = CC.series()
    dims = [int(d) for d in s["dims"]]
    DT = int(s["DT"])
    out = dict(s=s, dims=dims, DT=DT)
    for key in ("smoothed", "raw"):
        ctx = scalar_context(gpu, dims)
        out[key] = series_of(gpu, ctx, list(s[key]))
        ctx.close()
    ref, rf, _ = oracle.track(list(s["smoothed"]), 2, 1, tag_mode=oracle.TAG_REFERENCE)
    out["oracle"] = (ref, [int(f) for f in rf])
    return out


def test_the_noise_matters(woven):
    """(else the push tests below would pass with the smoothing left out)"""
    assert len(woven["smoothed"][0]) > 0 and not same_records(woven["smoothed"][0], woven["raw"][0])


@pytest.mark.parametrize("on_device", [0, 1, 2])
def test_push_smooths_like_the_reference(gpu, woven, on_device):
    s = woven["s"]
    ctx = scalar_context(gpu, woven["dims"])
    ctx.set_spatial_smoothing(float(s["sigma"]), int(s["ksize"]))
    recs, factors = series_of(gpu, ctx, list(s["raw"]), on_device)
    exp_recs, exp_factors = woven["smoothed"]
    assert factors == exp_factors == woven["oracle"][1]
    assert same_records(recs, exp_recs)
    assert_records_equal(as_fixture(recs), woven["oracle"][0], coord_tol=0.0, what=f"smoothed push, on_device {on_device}")
    # switched off again: the raw series' records
    ctx.set_spatial_smoothing(0.0, 0)
    recs, factors = series_of(gpu, ctx, list(s["raw"]), on_device)
    assert factors == woven["raw"][1] and same_records(recs, woven["raw"][0])
    ctx.close()


def test_vector_push_is_refused_while_smoothing(gpu):
    ctx = gpu.Context(2)
    ctx.set_mesh(([1, 1], [14, 10]), ([1, 1], [14, 10]), ([0, 0], [16, 12]))
    ctx.set_options(jacobian_symmetric=0, derive_jacobian=1)
    ctx.set_spatial_smoothing(1.0, 3)
    V = np.random.default_rng(3).uniform(-1, 1, size=(12, 16, 2))
    with pytest.raises(gpu.FtkxError) as e:
        ctx.push_slice(0, V)
    assert e.value.code == gpu._lib.E_UNSUPPORTED
    ctx.set_spatial_smoothing(0.0, 0)
    ctx.push_slice(0, V)
    ctx.close()


def test_push_3d_against_conv3D(gpu, oracle, ctx3):
    dims, DT, sigma, ksize = (17, 13, 11), 4, 1.0, 3
    rng = np.random.default_rng(29)
    raw = [oracle.synthetic("moving_extremum_3d", dims, k, DT, [8.25, 6.375, 5.125], [0.5, 0.25, 0.125]) + rng.uniform(-0.05, 0.05, size=tuple(reversed(dims))) for k in range(DT)]
    w = gpu.gaussian_kernel(3, sigma, ksize)
    smoothed = [device_conv(ctx3, a, w) for a in raw]
    for a, sm in zip(raw, smoothed):
        assert np.array_equal(sm.view(np.uint64), CC.conv(a, w).view(np.uint64))
    B = scalar_context(gpu, dims)
    exp_recs, exp_factors = series_of(gpu, B, smoothed)
    B.close()
    assert len(exp_recs) > 0
    for on_device in (0, 2):
        A = scalar_context(gpu, dims)
        A.set_spatial_smoothing(sigma, ksize)
        recs, factors = series_of(gpu, A, raw, on_device)
        A.close()
        assert factors == exp_factors and same_records(recs, exp_recs), on_device


# ---- the tracker -----------------------------------------------------------------------------------------------------------------------------
def tracked(gpu, slices, dims, smoothing=None, device=False, vector_push=False):
    import torch
    tr = gpu.CriticalPointTracker2DRegular()
    tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
    tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
    tr.set_domain([2, 2], [d - 3 for d in dims]); tr.set_array_domain([0, 0], list(dims))
    if smoothing:
        tr.set_spatial_smoothing(*smoothing)
    tr.initialize()
    if vector_push:
        try:
            tr.push_vector_field_snapshot(np.zeros((dims[1], dims[0], 2)))
        finally:
            tr.close()
        return None
    for k, a in enumerate(slices):
        if device:
            a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            torch.cuda.synchronize()
        tr.push_scalar_field_snapshot(a)
        if k:
            tr.advance_timestep()
    tr.update_timestep()
    recs, o, ts = tr.get_critical_points()
    tr.finalize()
    curves, loop = tr.get_traced_critical_points()
    tr.close()
    return recs, o, ts, [c.tolist() for c in curves], loop.tolist()


def test_tracker_smooths_in_front_of_the_sweep(gpu, woven):
    s = woven["s"]
    exp = tracked(gpu, list(s["smoothed"]), woven["dims"])
    assert len(exp[0]) > 0 and len(exp[3]) > 0
    for device in (False, True):
        got = tracked(gpu, list(s["raw"]), woven["dims"], smoothing=(float(s["sigma"]), int(s["ksize"])), device=device)
        assert same_records(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
        assert got[3] == exp[3] and got[4] == exp[4]
    with pytest.raises(gpu.FtkxError) as e:
        tracked(gpu, None, woven["dims"], smoothing=(1.0,), vector_push=True)          # (ksize: the default, 3)
    assert e.value.code == gpu._lib.E_UNSUPPORTED


# ---- several ranks: a slab's halo comes from slices that are smoothed already -----------------------------------------------------------
def slab_trackers(gpu, slices, dims, world, smoothing):
    """one tracker per rank and thread over the in-process hub on one device (tests/test_gpu_slab_host.py); -> rank 0's gathered points and curves"""
    import threading
    from ftk_amd import tslab, _lib
    L = _lib.load()
    nt = len(slices)
    hub = L.ftkx_slab_hub_create(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            tr = gpu.CriticalPointTracker2DRegular()
            tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
            tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
            tr.set_domain([2, 2], [d - 3 for d in dims]); tr.set_array_domain([0, 0], list(dims))
            if smoothing:
                tr.set_spatial_smoothing(*smoothing)
            tr.initialize()
            tr.set_slab_hub(hub, r, nt)
            t0, t1 = tslab.slab_range(nt, world, r)
            for k, t in enumerate(range(t0, t1)):
                tr.push_scalar_field_snapshot(slices[t])
                if k:
                    tr.advance_timestep()
                if t == t1 - 1:
                    tr.update_timestep()
            tr.finalize()
            curves, loop = tr.get_traced_critical_points()
            out[r] = (tr.get_critical_points(), [c.tolist() for c in curves], loop.tolist())
            tr.close()
        except BaseException as e:      # noqa: BLE001
            errs.append((r, e))
            L.ftkx_slab_hub_abort(hub)

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not [t for t in th if t.is_alive()] and not errs, errs
    L.ftkx_slab_hub_destroy(hub)
    return out[0]


def by_tag_points(points):
    recs, o, ts = points
    k = np.argsort(recs["tag"], kind="stable")
    return np.ascontiguousarray(recs[k]).tobytes(), o[k].tolist(), ts[k].tolist()


@pytest.mark.parametrize("case", ["plain_31x37", "compact_64x40"])
def test_slab_trackers_smooth_once(gpu, oracle, woven, case):
    """Two and three ranks with smoothing, raw slices in: the points and curves of ONE tracker handed the smoothed slices.  The 31-wide mesh
    has no summarised masks, so every rank takes its upper neighbour's first slice over whole (slab.cpp, the plain way: a push of the
    library's own of an array that is smoothed already); the 64-wide one goes the compact way (masks, request, patches of smoothed slices)."""
    if case == "plain_31x37":
        s = woven["s"]
        dims, raw, smoothed, smoothing = woven["dims"], list(s["raw"]), list(s["smoothed"]), (float(s["sigma"]), int(s["ksize"]))
    else:
        dims, DT, smoothing = [64, 40], 6, (1.0, 3)
        rng = np.random.default_rng(41)
        raw = [oracle.synthetic("woven", dims, k, DT) + rng.uniform(-0.05, 0.05, size=(dims[1], dims[0])) for k in range(DT)]
        w = gpu.gaussian_kernel(2, *smoothing)
        smoothed = [CC.conv(a, w) for a in raw]
    exp = tracked(gpu, smoothed, dims)
    unsmoothed = tracked(gpu, raw, dims)
    assert len(exp[3]) > 0 and not same_records(exp[0], unsmoothed[0])
    exp_points = by_tag_points(exp[:3])
    exp_curves = sorted(zip(map(tuple, exp[3]), exp[4]))
    for world in (2, 3):
        points, curves, loop = slab_trackers(gpu, raw, dims, world, smoothing)
        assert by_tag_points(points) == exp_points, (case, world)
        assert sorted(zip(map(tuple, curves), loop)) == exp_curves, (case, world)
