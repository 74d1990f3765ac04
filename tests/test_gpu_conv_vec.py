"""Spatial smoothing of vector snapshots on the GPU, every component as the scalar field it is (ftk_amd/csrc/conv_vec_kernels.hip).  The rule
has no tolerance: ftkx_conv2D_vec / ftkx_conv3D_vec / ftkx_conv_planar give, byte for byte, what ftkx_conv2D / ftkx_conv3D give per plane,
interleaved -- held here to the reference's own outputs (the fixtures of tests/golden/conv/ fed as components S, 2 S, S / 2), to the numpy
restatement on either side of every tile edge, and to the scalar kernel itself.  Then ftkx_set_vector_smoothing through every push form:
a context that smooths raw vector snapshots must give what a context gives that is handed the host-smoothed arrays -- resolution,
factors, records and the resident array itself -- and the trackers on top of it."""
import ctypes as C

import numpy as np
import pytest

import conv_cases as CC
import conv_vec_cases as VC

pytestmark = pytest.mark.gpu

SIGMA, KSIZE = 1.0, 3


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


@pytest.fixture(scope="module")
def ctxs(gpu):
    c = {2: gpu.Context(2), 3: gpu.Context(3)}
    yield c
    for v in c.values():
        v.close()


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
PAD = 8      # doubles of canary on either side of the output


def device_conv_vec(ctx, V, w, planar=False, f32=False):
    """V: (..., nd) -> what the entry writes, on the host; the output lies between canaries, the inputs are checked to be unchanged"""
    import torch
    nd = V.shape[-1]
    dt = np.float32 if f32 else np.float64
    host = [np.ascontiguousarray(V[..., c], dtype=dt) for c in range(nd)] if planar else [np.ascontiguousarray(V, dtype=dt)]
    src = [torch.from_numpy(a).cuda() for a in host]
    buf = torch.full((V.size + 2 * PAD,), 777.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dims = list(reversed(V.shape[:-1]))
    if planar:
        ctx.conv_planar([s.data_ptr() for s in src], dims, w, w.shape[0], buf.data_ptr() + 8 * PAD, f32=f32)
    else:
        ctx.conv_vec(src[0].data_ptr(), dims, w, w.shape[0], buf.data_ptr() + 8 * PAD, f32=f32)
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == 777.0) and np.all(got[-PAD:] == 777.0), "a canary was written"
    for s, a in zip(src, host):
        assert np.array_equal(s.cpu().numpy().view(np.uint32 if f32 else np.uint64), a.view(np.uint32 if f32 else np.uint64)), "an input was written"
    return got[PAD:-PAD].reshape(V.shape)


def device_conv(ctx, a, w):
    """the scalar kernel on one plane"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    out = torch.full(a.shape, 777.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dims = list(reversed(a.shape))
    if a.ndim == 2:
        ctx.conv2D(src.data_ptr(), dims[0], dims[1], w, w.shape[0], out.data_ptr())
    else:
        ctx.conv3D(src.data_ptr(), dims[0], dims[1], dims[2], w, w.shape[0], out.data_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("name", CC.fixture_names())
def test_fixtures_as_components(gpu, ctxs, name, planar):
    """the reference's own outputs: components (S, 2 S[, S / 2]) give (O, 2 O[, O / 2]) as 64-bit integers"""
    f = CC.load(name)
    V, O = VC.fixture_vector(f)
    got = device_conv_vec(ctxs[int(f["nd"])], V, f["weights"], planar=planar)
    assert np.array_equal(got.view(np.uint64), O.view(np.uint64)), name


@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_border_shapes(gpu, ctxs, ksize):
    """either side of the tile edges, all five sizes, interleaved and planar, double and float: the restatement per component, components
    that never mix (Inf in one, NaN in another), and the scalar kernel per plane byte for byte"""
    special = 0
    for shape in VC.SHAPES_2D + VC.SHAPES_3D:
        nd = len(shape)
        ctx = ctxs[nd]
        w = gpu.gaussian_kernel(nd, 0.75 + 0.25 * ksize, ksize)
        assert np.array_equal(w.view(np.uint64), VC.weights(nd, ksize).view(np.uint64))
        for f32 in (False, True):
            V, clean = VC.shape_vector(shape, ksize, f32)
            special += int(not np.isfinite(V).all())
            per_plane = np.stack([device_conv(ctx, V[..., c], w) for c in range(nd)], axis=-1)
            for planar in (False, True):
                got = device_conv_vec(ctx, V, w, planar, f32)
                VC.check_against_restatement(got, V, clean, w, (shape, ksize, planar, f32))
                assert np.array_equal(got.view(np.uint64), per_plane.view(np.uint64)), (shape, ksize, planar, f32)
    assert special == 4


def test_argument_errors(gpu, ctxs):
    import torch
    a = torch.zeros(256, dtype=torch.float64, device="cuda"); b = torch.zeros(256, dtype=torch.float64, device="cuda")
    w = np.full(729, 1.0 / 729)
    ctx2, ctx3 = ctxs[2], ctxs[3]
    L, E = ctx2._L, gpu._lib.E_INVALID
    p, q, wp = a.data_ptr(), b.data_ptr(), w.ctypes.data
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)      # noqa: E731
    for f in (L.ftkx_conv2D_vec, L.ftkx_conv2D_vec_f32):
        assert f(ctx2._h, p, 8, 8, wp, 4, q) == E and f(ctx2._h, p, 8, 8, wp, 11, q) == E and f(ctx2._h, p, 8, 8, wp, 0, q) == E      # ksize
        assert f(ctx2._h, p, 0, 8, wp, 3, q) == E and f(ctx2._h, p, 8, -1, wp, 3, q) == E                                            # extents
        assert f(ctx2._h, None, 8, 8, wp, 3, q) == E and f(ctx2._h, p, 8, 8, None, 3, q) == E and f(ctx2._h, p, 8, 8, wp, 3, None) == E
        assert f(ctx2._h, p, 8, 8, wp, 3, p) == E                                                                                    # in place
    assert L.ftkx_conv2D_vec(ctx2._h, p, 8, 4, wp, 3, p + 8 * 63) == E and L.ftkx_conv2D_vec(ctx2._h, p + 8 * 63, 8, 4, wp, 3, p) == E # overlapping
    assert L.ftkx_conv3D_vec(ctx3._h, p, 4, 4, 4, wp, 2, q) == E and L.ftkx_conv3D_vec(ctx3._h, p, 4, 4, 0, wp, 3, q) == E
    assert L.ftkx_conv_planar(ctx2._h, 2, ptrs(p, None), 8, 8, 1, wp, 3, q) == E and L.ftkx_conv_planar(ctx2._h, 2, None, 8, 8, 1, wp, 3, q) == E
    assert L.ftkx_conv_planar(ctx2._h, 4, ptrs(p, p, p, p), 4, 4, 1, wp, 3, q) == E
    assert L.ftkx_conv_planar(ctx2._h, 2, ptrs(p, q + 8 * 100), 8, 8, 1, wp, 3, q) == E                                                # a plane overlapping out
    assert L.ftkx_conv_planar_f32(ctx2._h, 2, ptrs(p, p), 8, 8, 1, wp, 6, q) == E
    assert L.ftkx_set_vector_smoothing(ctx2._h, 1.0, 4) == E and L.ftkx_set_vector_smoothing(ctx2._h, -1.0, 3) == E and L.ftkx_set_vector_smoothing(ctx2._h, 1.0, 11) == E
    assert L.ftkx_set_vector_smoothing(ctx2._h, 0.0, 0) == 0
    ms = (C.c_double * 2)()
    assert L.ftkx_debug_conv_vec_relaunch(ctx2._h, 2, ptrs(p), 0, 0, 8, 8, 1, wp, 3, q, 0, ms) == E and L.ftkx_debug_conv_vec_relaunch(ctx2._h, 2, ptrs(p), 0, 0, 8, 8, 1, wp, 3, q, 2, None) == E
    assert L.ftkx_conv_planar(ctx2._h, 2, ptrs(p, p), 8, 8, 1, wp, 3, q) == 0                                                          # planes may be one another
    assert len(ctx2.debug_conv_vec_relaunch([p], (8, 8), w[:9], 3, q, 2)) == 2
    assert len(ctx3.debug_conv_vec_relaunch([p, p, p], (4, 4, 4), w[:27], 3, q, 2, planar=True)) == 2
    assert ctx2.conv_vec_counts() == (0, 0, 0) and ctx3.conv_vec_counts() == (0, 0, 0)          # (the counters are the pushes')


# ---- 2. the push path ----------------------------------------------------------------------------------------------------------------------
def vector_context(gpu, dims, smoothing=False, adjust=False, temporal=False):
    nd = len(dims)
    dom = ([1] * nd, [d - 2 for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=0, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
    if smoothing:
        ctx.set_vector_smoothing(SIGMA, KSIZE)
    if adjust:
        ctx.set_perturbation(0.002, 20240607); ctx.set_clamp(-0.3, 0.28)
    if temporal:
        ctx.set_temporal_smoothing(1.0, 3, 0)
    return ctx


def same_records(a, b):
    return len(a) == len(b) and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def outcome(gpu, ctx, ts, dims):
    """what a context holds and gives for its resident slices ts: per slice (resolution, max |v|) and the resident array as the patches of
    EVERY core cell see it (corner - 2 .. corner + 3 on every axis, clamped: all of the array), then factors and records of one pass"""
    import torch
    ncells = int(np.prod([d - 2 for d in dims]))
    cells = torch.arange(ncells, dtype=torch.int64, device="cuda")
    res = [ctx.slice_resolution(t) for t in ts]
    resident = [ctx.gather_patches(t, cells, torch).cpu().numpy().tobytes() for t in ts]
    scopes = [gpu.SCOPE_BOTH if i + 1 < len(ts) else gpu.SCOPE_ORDINAL for i in range(len(ts))]
    recs, factors, _ = ctx.sweep_series(list(ts), scopes)
    return dict(ts=list(ts), res=res, resident=resident, factors=[int(f) for f in factors], recs=recs)


def assert_same_outcome(got, exp, what):
    assert got["ts"] == exp["ts"], what
    assert got["res"] == exp["res"], what
    assert got["resident"] == exp["resident"], (what, "the resident arrays differ")
    assert got["factors"] == exp["factors"], what
    assert same_records(got["recs"], exp["recs"]), what


def gyre2d():
    """a noisy double_gyre, 33 x 17 over 4 steps; every value a float16 (so float32 and float16 pushes carry the same field)"""
    import torch
    from ftk_amd import synthetic
    rng = np.random.default_rng(77)
    dims = (33, 17)
    return dims, [(synthetic.double_gyre(dims, k, torch, "cpu").numpy() + rng.uniform(-0.03, 0.03, size=(17, 33, 2))).astype(np.float16).astype(np.float64) for k in range(4)]


def field3d():
    """a small noisy 3D vector series, 17 x 13 x 11 over 3 steps; every value a float16"""
    rng = np.random.default_rng(78)
    dims = (17, 13, 11)
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    out = []
    for t in range(3):
        u = np.sin(0.5 * x + 0.3 * t) + 0.3 * np.cos(0.4 * z)
        v = np.cos(0.45 * y - 0.2 * t) + 0.3 * np.sin(0.5 * x)
        w = np.sin(0.6 * z + 0.1 * t) - 0.3 * np.cos(0.35 * y)
        out.append((np.stack([u, v, w], axis=-1) * 0.2 + rng.uniform(-0.03, 0.03, size=x.shape + (3,))).astype(np.float16).astype(np.float64))
    return dims, out


def push_all(ctx, V, temporal):
    ts = []
    for t, a in enumerate(V):
        if temporal:
            ts.append(ctx.temporal_push(a, is_vector=True))
        else:
            ctx.push_slice(t, a); ts.append(t)
    while temporal:
        t = ctx.temporal_flush()
        if t < 0:
            break
        ts.append(t)
    return [t for t in ts if t >= 0]


@pytest.fixture(scope="module")
def series(gpu):
    """per mesh: the raw series, the host-smoothed one (conv_cases.conv per component under the library's own weights), and what a context
    WITHOUT the setting gives for either -- plain, with perturbation and clamp, and through the temporal filter -- computed once"""
    out = {}
    for name, (dims, raw) in (("gyre2d", gyre2d()), ("field3d", field3d())):
        nd = len(dims)
        w = gpu.gaussian_kernel(nd, SIGMA, KSIZE)
        smoothed = [VC.conv_vec(a, w) for a in raw]
        m = dict(dims=dims, nd=nd, raw=raw, smoothed=smoothed)
        for adjust in (False, True):
            for temporal in (False, True):
                for key, arrays in (("smoothed", smoothed), ("raw", raw)):
                    ctx = vector_context(gpu, dims, adjust=adjust, temporal=temporal)
                    ts = push_all(ctx, arrays, temporal)
                    m[(key, adjust, temporal)] = outcome(gpu, ctx, ts, dims)
                    assert ctx.conv_vec_counts() == (0, 0, 0)
                    ctx.close()
        out[name] = m
    return out


@pytest.mark.parametrize("mesh", ["gyre2d", "field3d"])
def test_the_noise_matters(series, mesh):
    """(else the push tests below would pass with the smoothing left out)"""
    m = series[mesh]
    for adjust in (False, True):
        for temporal in (False, True):
            s, r = m[("smoothed", adjust, temporal)], m[("raw", adjust, temporal)]
            assert len(s["recs"]) > 0 and len(r["recs"]) > 0 and not same_records(s["recs"], r["recs"]), (mesh, adjust, temporal)
            assert s["resident"] != r["resident"]


FORMS = ["host64", "dev1", "dev2", "f32", "f32_dev1", "f16", "f16_dev1", "planar64", "planar64_dev1", "planar32", "planar32_dev2", "temporal", "temporal_dev1", "temporal_f32",
         "temporal_f16", "temporal_planar", "temporal_planar32_dev1"]


def push_form(gpu, ctx, t, a, form):
    """one raw snapshot into context `ctx` by the named form -> the timestep that became resident (-1: none yet).  Device sources are
    checked to be unchanged and then overwritten: the context owns what it needs (never adopted)"""
    import torch
    parts = form.split("_")
    temporal = parts[0] == "temporal"
    if temporal:
        parts = parts[1:] or ["host64"]
    dev = 1 if "dev1" in parts else 2 if "dev2" in parts else 0
    kind = parts[0] if parts[0] not in ("dev1", "dev2") else "host64"
    dtype = {"host64": np.float64, "f32": np.float32, "f16": np.float16, "planar64": np.float64, "planar32": np.float32, "planar": np.float64}[kind]
    planar = kind.startswith("planar")
    host = [np.ascontiguousarray(a[..., c], dtype=dtype) for c in range(a.shape[-1])] if planar else [np.ascontiguousarray(a, dtype=dtype)]
    given = [torch.from_numpy(h.copy()).cuda() for h in host] if dev else [h.copy() for h in host]
    torch.cuda.synchronize()
    L, h = ctx._L, ctx._h
    out = C.c_int(-1)
    if planar:
        if temporal:
            out.value = ctx.temporal_push_planar(given, on_device=dev if dev else None)
        else:
            ctx.push_slice_planar(t, given, on_device=dev if dev else None)
    elif temporal:
        out.value = ctx.temporal_push(given[0], is_vector=True, on_device=dev if dev else None, keep_dtype=True)
    elif dev == 2:
        assert kind == "host64"
        ctx._ck(L.ftkx_push_slice(h, t, given[0].data_ptr(), None, None, 2))
    else:
        ctx.push_slice(t, given[0], keep_dtype=True)
    for g, hh in zip(given, host):
        now = g.cpu().numpy() if dev else g
        assert now.tobytes() == hh.tobytes(), "a pushed array was written"
        g[...] = 7
    torch.cuda.synchronize()
    return out.value if temporal else t


@pytest.mark.parametrize("adjust", [False, True], ids=["plain", "perturb_clamp"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mesh", ["gyre2d", "field3d"])
def test_smoothed_push_is_the_push_of_the_smoothed_array(gpu, series, mesh, form, adjust):
    """context A has the setting on and receives the raw array by `form`; context B (the fixture's) has it off and received the
    host-smoothed array: resolution, resident array, factors and records agree bit for bit; widen -> smooth -> perturb -> clamp -> ring"""
    m = series[mesh]
    temporal = form.startswith("temporal")
    A = vector_context(gpu, m["dims"], smoothing=True, adjust=adjust, temporal=temporal)
    before = (A.planar_counts(), A.f32_counts())
    ts = [push_form(gpu, A, t, a, form) for t, a in enumerate(m["raw"])]
    while temporal:
        t = A.temporal_flush()
        if t < 0:
            break
        ts.append(t)
    ts = [t for t in ts if t >= 0]
    counts = A.conv_vec_counts()
    n = len(m["raw"])
    planar, f32 = "planar" in form, "32" in form
    assert counts == ((0, n, n if f32 else 0) if planar else (n, 0, n if f32 else 0)), (form, counts)
    assert (A.planar_counts(), A.f32_counts()) == before, "a concat, widen or scalar convolution launch beside the one kernel"
    got = outcome(gpu, A, ts, m["dims"])
    A.close()
    assert_same_outcome(got, m[("smoothed", adjust, temporal)], (mesh, form, adjust))


def test_switched_off_again_and_scalar_pushes_pass_it_by(gpu, series):
    m = series["gyre2d"]
    A = vector_context(gpu, m["dims"], smoothing=True)
    A.set_vector_smoothing(0.0, 0)
    for t, a in enumerate(m["raw"]):
        A.push_slice(t, a)
    assert A.conv_vec_counts() == (0, 0, 0)
    assert_same_outcome(outcome(gpu, A, range(len(m["raw"])), m["dims"]), m[("raw", False, False)], "off again")
    A.close()
    # a scalar context with ONLY the vector setting: its pushes are plain copies
    import torch
    S = [np.ascontiguousarray(a[..., 0]) for a in m["raw"]]
    outs = []
    for on in (False, True):
        ctx = gpu.Context(2)
        dom = ([2, 2], [d - 4 for d in m["dims"]])
        ctx.set_mesh(dom, dom, ([0, 0], list(m["dims"])))
        ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
        if on:
            ctx.set_vector_smoothing(SIGMA, KSIZE)
        for t, s in enumerate(S):
            ctx.push_scalar_slice(t, s)
        outs.append(([ctx.slice_resolution(t) for t in range(len(S))], ctx.conv_vec_counts()))
        ctx.close()
    assert outs[0] == outs[1] and outs[1][1] == (0, 0, 0)


def test_refusals(gpu, series):
    m = series["gyre2d"]
    U = gpu._lib.E_UNSUPPORTED
    V = m["raw"][0]
    J = np.zeros(V.shape[:2] + (2, 2)); S = np.zeros(V.shape[:2])
    ctx = vector_context(gpu, m["dims"], smoothing=True)

    def refused(code, call):
        with pytest.raises(gpu.FtkxError) as e:
            call()
        assert e.value.code == code, str(e.value)

    refused(U, lambda: ctx.push_slice(0, V, J, None))
    refused(U, lambda: ctx.push_slice(0, V, None, S))
    refused(U, lambda: ctx.push_slice_planar(0, [np.ascontiguousarray(V[..., c]) for c in range(2)], J, None))
    assert ctx.conv_vec_counts() == (0, 0, 0)
    ctx.push_slice(0, V)                                   # the context goes on
    assert ctx.conv_vec_counts() == (1, 0, 0)
    # both settings: the vector one decides for vectors; the scalar one alone keeps refusing them
    ctx.set_spatial_smoothing(1.0, 3)
    ctx.push_slice(1, V)
    ctx.set_vector_smoothing(0.0, 0)
    refused(U, lambda: ctx.push_slice(2, V))
    ctx.close()


# ---- 3. the trackers (the Python classes drive the C++ tracker through its C handle) -----------------------------------------------------------
def make_tracker(gpu, dims, smoothing, **kw):
    tr = gpu.CriticalPointTracker2DRegular(**kw)
    tr.set_scalar_field_source(gpu.SOURCE_NONE); tr.set_vector_field_source(gpu.SOURCE_GIVEN)
    tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(False)
    tr.set_domain([1, 1], [d - 2 for d in dims]); tr.set_array_domain([0, 0], list(dims))
    tr.set_tag_mode(gpu.TAG_REFERENCE)
    if smoothing:
        tr.set_vector_spatial_smoothing(SIGMA, KSIZE)
    return tr


def push_step(tr, V, how):
    import torch
    if how == "components":
        tr.push_vector_field_components([np.ascontiguousarray(V[..., c]) for c in range(V.shape[-1])])
    elif how == "device":
        x = torch.from_numpy(np.ascontiguousarray(V)).cuda()
        torch.cuda.synchronize()
        tr.push_vector_field_snapshot(x)
        x.fill_(7.0); torch.cuda.synchronize()
    elif how == "float32":
        tr.push_vector_field_snapshot(np.ascontiguousarray(V, dtype=np.float32))
    else:
        tr.push_vector_field_snapshot(np.ascontiguousarray(V))


def tracked(gpu, steps, dims, smoothing, how="snapshot", temporal=False, **kw):
    tr = make_tracker(gpu, dims, smoothing, **kw)
    if temporal:
        tr.set_temporal_smoothing(1.0, 3)
    tr.initialize()
    n = 0

    def arrived():
        nonlocal n
        if n:
            tr.advance_timestep()
        n += 1

    for V in steps:
        push_step(tr, V, how)
        if tr.snapshots_from_last_push():
            arrived()
    while temporal and tr.flush_temporal_smoothing():
        arrived()
    tr.update_timestep()
    recs, o, ts = tr.get_critical_points()
    tr.finalize()
    curves, loop = tr.get_traced_critical_points()
    tr.close()
    return recs, o, ts, [c.tolist() for c in curves], loop.tolist()


def assert_same_tracking(got, exp, what):
    assert same_records(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), what
    assert got[3] == exp[3] and got[4] == exp[4], what


@pytest.fixture(scope="module")
def tracked_smoothed(gpu, series):
    m = series["gyre2d"]
    exp = tracked(gpu, m["smoothed"], m["dims"], False)
    raw = tracked(gpu, m["raw"], m["dims"], False)
    assert len(exp[0]) > 0 and len(exp[3]) > 0 and not same_records(exp[0], raw[0])
    return exp


@pytest.mark.parametrize("how", ["snapshot", "device", "float32", "components"])
def test_tracker_smooths_in_front_of_the_sweep(gpu, series, tracked_smoothed, how):
    m = series["gyre2d"]
    assert_same_tracking(tracked(gpu, m["raw"], m["dims"], True, how), tracked_smoothed, how)


def test_tracker_with_the_device_listed_twice(gpu, series):
    """a halo snapshot is smoothed on both contexts that receive it, alike"""
    m = series["gyre2d"]
    exp = tracked(gpu, m["smoothed"], m["dims"], False, device_ids=[0, 0])
    assert len(exp[0]) > 0
    assert_same_tracking(tracked(gpu, m["raw"], m["dims"], True, device_ids=[0, 0]), exp, "multi-device")


def test_tracker_with_temporal_smoothing(gpu, series):
    m = series["gyre2d"]
    exp = tracked(gpu, m["smoothed"], m["dims"], False, temporal=True)
    assert len(exp[0]) > 0
    for how in ("snapshot", "components"):
        assert_same_tracking(tracked(gpu, m["raw"], m["dims"], True, how, temporal=True), exp, ("temporal", how))


def test_tracker_refuses_field_data(gpu, series):
    m = series["gyre2d"]
    V = m["raw"][0]
    tr = make_tracker(gpu, m["dims"], True)
    tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_jacobian_field_source(gpu.SOURCE_GIVEN)
    tr.initialize()
    with pytest.raises(gpu.FtkxError) as e:
        tr.push_field_data_snapshot(np.zeros(V.shape[:2]), V, np.zeros(V.shape[:2] + (2, 2)))
    assert e.value.code == gpu._lib.E_UNSUPPORTED
    tr.close()


def slab_trackers(gpu, steps, dims, world, smoothing, components):
    """one tracker per rank and thread over the in-process hub on one device (the pattern of tests/test_gpu_conv.py) -> rank 0's points, curves"""
    import threading
    from ftk_amd import tslab, _lib
    L = _lib.load()
    nt = len(steps)
    hub = L.ftkx_slab_hub_create(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            tr = make_tracker(gpu, dims, smoothing)
            tr.initialize()
            tr.set_slab_hub(hub, r, nt)
            t0, t1 = tslab.slab_range(nt, world, r)
            for k, t in enumerate(range(t0, t1)):
                push_step(tr, steps[t], "components" if components else "snapshot")
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


def test_two_slab_ranks_smooth_once(gpu, series, tracked_smoothed):
    """two in-process slab ranks with the setting on, raw snapshots in: the points and curves of ONE tracker handed the smoothed arrays (the
    upper neighbour's first slice arrives smoothed and is not smoothed again)"""
    m = series["gyre2d"]
    exp_points = by_tag_points(tracked_smoothed[:3])
    exp_curves = sorted(zip(map(tuple, tracked_smoothed[3]), tracked_smoothed[4]))
    for components in (False, True):
        points, curves, loop = slab_trackers(gpu, m["raw"], m["dims"], 2, True, components)
        assert by_tag_points(points) == exp_points, components
        assert sorted(zip(map(tuple, curves), loop)) == exp_curves, components
