"""Perturbation and clamp on the GPU (ftk_amd/csrc/adjust_kernels.hip, adjust_steps.hpp): the bare kernel against the host build of the very
header it is compiled from, bit for bit; then ftkx_set_perturbation / ftkx_set_clamp through every way a snapshot becomes resident -- the
slice read back through the patches the halo exchange uses and held, byte for byte, to widen -> conv restatement -> host adjust -- the
temporal filter behind them, the records of swept series against a second context that was pushed the host-adjusted arrays, the tracker
alone and as two slab ranks, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import adjust_cases as AC
import conv_cases as CC
import temporal_cases as TC
from test_gpu_temporal import Mesh, bits

pytestmark = pytest.mark.gpu

SIGMA, SEED, CLAMP = 0.05, 2024, (-0.97, 0.96)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    AC.host()
    return ftk_amd


# ---- the bare kernel --------------------------------------------------------------------------------------------------------------------------
def device_adjust(ctx, x, src_off, dst_off, in_place, sigma, clamp):
    """x (float64 / float32, host) from `src_off` elements behind a 16-byte border to `dst_off` doubles behind one, canaries on both sides of
    the destination; in_place: the destination is the source.  The source must come back unchanged (out of place)"""
    import torch
    count = x.size
    f32 = x.dtype == np.float32
    dt = torch.float32 if f32 else torch.float64
    pad = 4
    if in_place:
        assert not f32
        buf = torch.full((2 * pad + dst_off + count,), 777.0, dtype=torch.float64, device="cuda")
        buf[pad + dst_off:pad + dst_off + count].copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        p = buf.data_ptr() + 8 * (pad + dst_off)
        ctx.adjust(p, count, p, sigma=sigma, seed=AC.SEED, t=AC.T, clamp=clamp)
        o = buf.cpu().numpy()
    else:
        src = torch.zeros(src_off + count, dtype=dt, device="cuda")
        src[src_off:].copy_(torch.from_numpy(x))
        keep = src.clone()
        buf = torch.full((2 * pad + dst_off + count,), 777.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.adjust(src.data_ptr() + src_off * x.itemsize, count, buf.data_ptr() + 8 * (pad + dst_off), sigma=sigma, seed=AC.SEED, t=AC.T, clamp=clamp, f32=f32)
        it = torch.int32 if f32 else torch.int64
        assert torch.equal(src.view(it), keep.view(it)), "the source was written"
        o = buf.cpu().numpy()
    at = pad + dst_off
    assert (o[:at] == 777.0).all() and (o[at + count:] == 777.0).all(), "a store outside the destination"
    return o[at:at + count]


@pytest.mark.parametrize("count", [c for c in AC.COUNTS if c > 0])
def test_kernel_is_the_host_header_bit_for_bit(gpu, count):
    """every count and offset of the host test's plan, clamp only / perturb only / both, FP64 out of place and in place, float32; the values
    hold NaN, +-0, +-inf and subnormals, where v_max_f64 / v_min_f64 would show.  This is also what establishes that sqrt and / of the
    build round on the MI355X as they do on the host"""
    ctx = gpu.Context(2)
    big = count > 2000
    x, xf = AC.values(count, 31 * count + 1, np.float64), AC.values(count, 31 * count + 2, np.float32)
    assert count < 8 or (np.isnan(x[:16]).any() and np.isnan(xf[:16]).any())
    worst = 0
    for mode, (perturb, clamp) in sorted(AC.MODES.items()):
        sigma, cl = (AC.SIGMA if perturb else 0.0), ((AC.LO, AC.HI) if clamp else None)
        exp, expf = AC.host_adjust(x, sigma, AC.SEED, AC.T, cl), AC.host_adjust(xf, sigma, AC.SEED, AC.T, cl)
        for src_off in range(4):
            for dst_off in range(2):
                if big and (src_off, dst_off) not in ((0, 0), (1, 1)):
                    continue
                got = [(device_adjust(ctx, xf, src_off, dst_off, False, sigma, cl), expf, "float32")]
                if src_off < 2:
                    got.append((device_adjust(ctx, x, src_off, dst_off, False, sigma, cl), exp, "float64"))
                if src_off == 0:
                    got.append((device_adjust(ctx, x, 0, dst_off, True, sigma, cl), exp, "in place"))
                for g, e, what in got:
                    differ = int((bits(g) != bits(e)).sum())
                    worst = max(worst, differ)
                    assert differ == 0, (count, mode, what, src_off, dst_off, differ, [(i, g[i], e[i]) for i in np.nonzero(bits(g) != bits(e))[0][:4]])
    print("count", count, "elements that differ from the host header:", worst)
    ctx.close()


def test_kernel_snapshot_seed_and_far_elements(gpu):
    """t and both words of the seed reach the kernel; so does sigma"""
    import torch
    ctx = gpu.Context(2)
    n = 513
    z = torch.zeros(n, dtype=torch.float64, device="cuda"); out = torch.empty_like(z)
    torch.cuda.synchronize()
    for sigma, seed, t in ((1.0, 1, 0), (1.0, 1, 1), (1.0, 1 + (1 << 32), 0), (1.0, (1 << 64) - 1, 2 ** 31 - 1), (3.5, 1, 0)):
        ctx.adjust(z.data_ptr(), n, out.data_ptr(), sigma=sigma, seed=seed, t=t)
        assert AC.same_bits(out.cpu().numpy(), AC.host_adjust(np.zeros(n), sigma, seed, t)), (sigma, seed, t)
    ctx.close()


# ---- pushes -----------------------------------------------------------------------------------------------------------------------------------
def pipeline(a, t, smooth_w=None, sigma=SIGMA, seed=SEED, clamp=CLAMP):
    """widen -> conv restatement -> host adjust, as the stream orders them"""
    x = np.ascontiguousarray(a).astype(np.float64)
    if smooth_w is not None:
        x = CC.conv(x, smooth_w)
    return AC.host_adjust(x, sigma, seed, t, clamp)


def push_and_read(mesh, t, a, on_device):
    """one scalar / vector push; a device source is checked to be unchanged and is overwritten at once: the context owns what it keeps"""
    import torch
    ctx = mesh.ctx
    if on_device:
        x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        before = x.clone()
        torch.cuda.synchronize()
        if mesh.vector:
            assert on_device == 1
            ctx.push_slice(t, x)
        else:
            ctx.push_scalar_slice(t, x, on_device=on_device)
        it = torch.int32 if a.dtype == np.float32 else torch.int64
        assert torch.equal(x.view(it), before.view(it)), "a pushed tensor was written"
        x.fill_(777.0)
        torch.cuda.synchronize()
    elif mesh.vector:
        ctx.push_slice(t, a)
    else:
        ctx.push_scalar_slice(t, a)
    return mesh.read(t)


@pytest.mark.parametrize("dims", [(33, 9), (33, 9, 9)])
def test_scalar_pushes_against_the_pipeline(gpu, dims):
    """on_device 0 / 1 / 2, float64 and float32, with and without spatial smoothing at ksize 3: the slice, and ONE adjust kernel of the kind
    the path calls for"""
    mesh = Mesh(gpu, dims, False)
    ctx = mesh.ctx
    raw = CC.random_input(tuple(reversed(dims)), 77 + len(dims))
    w = gpu.gaussian_kernel(len(dims), 1.0, 3)
    kind_of = {(np.float32, False): 0, (np.float32, True): 1, (np.float64, True): 1}       # index into (from_float, in_place, out_of_place)
    t = 0
    for sigma, clamp in ((SIGMA, CLAMP), (SIGMA, None), (0.0, CLAMP)):
        ctx.set_perturbation(sigma, SEED)
        ctx.set_clamp(*(clamp or (None, None)))
        for smooth in (False, True):
            ctx.set_spatial_smoothing(1.0, 3 if smooth else 0)
            for dtype in (np.float64, np.float32):
                a = raw.astype(dtype)
                for on_device in (0, 1, 2):
                    t += 3
                    before = ctx.adjust_counts()
                    plain = ctx.f32_counts()
                    got = push_and_read(mesh, t, a, on_device)
                    exp = pipeline(a, t, w if smooth else None, sigma, SEED, clamp)
                    assert np.array_equal(bits(got), bits(exp)), (dims, sigma, clamp, smooth, dtype, on_device)
                    kind = kind_of.get((dtype, smooth), 1 if on_device == 0 else 2)
                    delta = [x - y for x, y in zip(ctx.adjust_counts(), before)]
                    assert delta == [int(k == kind) for k in range(3)], (delta, kind, smooth, dtype, on_device)
                    assert ctx.f32_counts()[0] == plain[0]                                   # the widen kernel did not run
                    ctx.drop_slice(t)
    assert not np.array_equal(bits(pipeline(raw, 5)), bits(raw)) and not np.array_equal(bits(pipeline(raw, 5)), bits(pipeline(raw, 6)))
    # both off again: the plain paths, and no adjust kernel
    ctx.set_perturbation(0.0, 0); ctx.set_clamp(); ctx.set_spatial_smoothing(0.0, 0)
    before = ctx.adjust_counts()
    for on_device in (0, 2):
        assert np.array_equal(bits(push_and_read(mesh, 1, raw, on_device)), bits(raw))
    assert np.array_equal(bits(push_and_read(mesh, 2, raw.astype(np.float32), 0)), bits(raw.astype(np.float32).astype(np.float64)))
    assert ctx.adjust_counts() == before
    mesh.close()


def test_settings_off_queue_no_adjust_kernel(gpu):
    """a context that never had a setting on, and one that had: all three counters stay where they were"""
    mesh = Mesh(gpu, (33, 9), False)
    a = CC.random_input((9, 33), 5)
    w = gpu.gaussian_kernel(2, 1.0, 3)
    for smooth in (False, True):
        mesh.ctx.set_spatial_smoothing(1.0, 3 if smooth else 0)
        for dtype in (np.float64, np.float32):
            for on_device in (0, 2):
                got = push_and_read(mesh, 1, a.astype(dtype), on_device)
                x = a.astype(dtype).astype(np.float64)
                assert np.array_equal(bits(got), bits(CC.conv(x, w) if smooth else x))
    assert mesh.ctx.adjust_counts() == (0, 0, 0)
    assert mesh.ctx.f32_counts() == (2, 2)
    mesh.close()


def test_vector_push_adjusts_every_component_by_its_flat_index(gpu):
    mesh = Mesh(gpu, (33, 9), True)
    ctx = mesh.ctx
    V = CC.random_input((9, 33, 2), 91)
    ctx.set_perturbation(SIGMA, SEED); ctx.set_clamp(*CLAMP)
    for t, (dtype, on_device, kind) in enumerate(((np.float64, 0, 1), (np.float64, 1, 2), (np.float32, 0, 0), (np.float32, 1, 0))):
        before = ctx.adjust_counts()
        got = push_and_read(mesh, t, V.astype(dtype), on_device)
        assert np.array_equal(bits(got), bits(pipeline(V.astype(dtype), t))), (dtype, on_device)
        assert [x - y for x, y in zip(ctx.adjust_counts(), before)] == [int(k == kind) for k in range(3)]
    mesh.close()


# ---- the temporal filter behind them ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 2])
@pytest.mark.parametrize("on_device", [0, 1])
def test_adjusted_snapshots_enter_the_ring(gpu, N, on_device):
    """K = 3: N = 5 emits five arrays, N = 2 the reference's short series (one).  Every emission and flush is the temporal restatement over
    the host-adjusted raw arrays, raw snapshot i being number t0 + i -- in a second series behind the first, the next unused timestep + i"""
    import torch
    dims, K, t0 = (33, 9), 3, 4
    mesh = Mesh(gpu, dims, False)
    ctx = mesh.ctx
    raw = [CC.random_input((9, 33), 300 + i) for i in range(N)]
    wt = gpu.gaussian_kernel1d(1.0, K)
    ws = gpu.gaussian_kernel(2, 1.0, 3)
    ctx.set_perturbation(SIGMA, SEED); ctx.set_clamp(*CLAMP)
    first = t0
    for smooth in (False, True):
        ctx.set_spatial_smoothing(1.0, 3 if smooth else 0)
        ctx.set_temporal_smoothing(1.0, K, first)
        for again in range(2):
            exp = TC.smooth_series([pipeline(a, first + i, ws if smooth else None) for i, a in enumerate(raw)], wt)
            assert len(exp) == (5 if N == 5 else 1)
            got = []
            for a in raw:
                x = torch.from_numpy(a).cuda() if on_device else a
                t = ctx.temporal_push(x, on_device=on_device if on_device else None)
                if on_device:
                    x.fill_(777.0); torch.cuda.synchronize()
                if t >= 0:
                    got.append((t, mesh.read(t)))
            while True:
                t = ctx.temporal_flush()
                if t < 0:
                    break
                got.append((t, mesh.read(t)))
            assert [t for t, _ in got] == list(range(first, first + len(exp))), (N, smooth, again)
            for (t, g), e in zip(got, exp):
                assert np.array_equal(bits(g), bits(e)), (N, smooth, again, t)
            first += len(exp)
    mesh.close()


# ---- records ------------------------------------------------------------------------------------------------------------------------------------
def scalar_context(gpu, dims):
    nd = len(dims)
    dom = ([2] * nd, [d - 3 for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
    return ctx


def swept(gpu, ctx, slices, ts=None):
    nt = len(slices)
    for t, a in enumerate(slices):
        ctx.push_scalar_slice(t, a)
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    recs, factors, _ = ctx.sweep_series(range(nt), scopes)
    return np.ascontiguousarray(recs).tobytes(), [int(f) for f in factors]


def series(gpu, case):
    import torch
    from ftk_amd import synthetic
    if case == "woven":
        dims, DT = (32, 32), 4
        raw = [synthetic.woven(dims, k, DT, torch, "cuda").cpu().numpy() for k in range(DT)]
        return dims, raw, 0.05, CLAMP
    dims, DT = (17, 16, 9), 3
    raw = [synthetic.moving_extremum(dims, k, [8.25, 8.375, 4.125], [0.5, 0.25, 0.125], torch, "cuda").cpu().numpy() for k in range(DT)]
    return dims, raw, 0.125, (-0.25, 140.0)


@pytest.mark.parametrize("case", ["woven", "moving_extremum_3d"])
def test_records_of_adjusted_series(gpu, case):
    dims, raw, sigma, clamp = series(gpu, case)
    B = scalar_context(gpu, dims)
    exp = swept(gpu, B, [AC.host_adjust(a, sigma, SEED, t, clamp) for t, a in enumerate(raw)])
    other = swept(gpu, B, [AC.host_adjust(a, sigma, SEED + 1, t, clamp) for t, a in enumerate(raw)])
    plain = swept(gpu, B, raw)
    B.close()
    assert len(exp[0]) > 0 and exp[0] != plain[0] and exp[0] != other[0]
    A = scalar_context(gpu, dims)
    A.set_perturbation(sigma, SEED); A.set_clamp(*clamp)
    assert swept(gpu, A, raw) == exp
    assert swept(gpu, A, raw) == exp                                    # the same timesteps pushed again: the same noise
    A.set_perturbation(sigma, SEED + 1)
    assert swept(gpu, A, raw) == other                                  # another seed, other records
    A.set_perturbation(0.0, 0); A.set_clamp()
    assert swept(gpu, A, raw) == plain
    A.close()


# ---- the tracker ------------------------------------------------------------------------------------------------------------------------------
def tracker_of(gpu, dims, adjust=None, **kw):
    tr = gpu.CriticalPointTracker2DRegular(**kw)
    tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
    tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
    tr.set_domain([2, 2], [d - 3 for d in dims]); tr.set_array_domain([0, 0], list(dims))
    if adjust:
        tr.set_perturbation(adjust[0], adjust[1])
        tr.set_clamp(*adjust[2])
    return tr


def tracked(gpu, slices, dims, adjust=None, device=False, **kw):
    import torch
    tr = tracker_of(gpu, dims, adjust, **kw)
    tr.initialize()
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
    return np.ascontiguousarray(recs).tobytes(), o.tolist(), ts.tolist(), [c.tolist() for c in curves], loop.tolist(), (recs, o, ts)


@pytest.fixture(scope="module")
def noisy_woven(gpu):
    """the conv fixture's noisy woven series (31 x 37 x 8) and what a plain tracker gives for its host-adjusted and its raw slices"""
    s = CC.series()
    dims = [int(d) for d in s["dims"]]
    raw = list(s["raw"])
    adjusted = [AC.host_adjust(a, SIGMA, SEED, t, CLAMP) for t, a in enumerate(raw)]
    return dict(dims=dims, raw=raw, exp=tracked(gpu, adjusted, dims), plain=tracked(gpu, raw, dims))


def test_tracker_adjusts_in_front_of_the_sweep(gpu, noisy_woven):
    exp = noisy_woven["exp"]
    assert len(exp[0]) > 0 and len(exp[3]) > 0 and exp[0] != noisy_woven["plain"][0]
    for device in (False, True):
        got = tracked(gpu, noisy_woven["raw"], noisy_woven["dims"], adjust=(SIGMA, SEED, CLAMP), device=device)
        assert got[:5] == exp[:5], device
    got = tracked(gpu, [a.astype(np.float32) for a in noisy_woven["raw"]], noisy_woven["dims"], adjust=(SIGMA, SEED, CLAMP))
    f32 = tracked(gpu, [AC.host_adjust(a.astype(np.float32), SIGMA, SEED, t, CLAMP) for t, a in enumerate(noisy_woven["raw"])], noisy_woven["dims"])
    assert got[:5] == f32[:5]
    # two contexts behind one tracker: a snapshot that both are handed gets the same noise in both
    got = tracked(gpu, noisy_woven["raw"], noisy_woven["dims"], adjust=(SIGMA, SEED, CLAMP), device_ids=[0, 0])
    assert by_tag_points(got[5]) == by_tag_points(exp[5]) and sorted(zip(map(tuple, got[3]), got[4])) == sorted(zip(map(tuple, exp[3]), exp[4]))
    # one array only
    tr = tracker_of(gpu, noisy_woven["dims"], adjust=(SIGMA, SEED, CLAMP))
    tr.set_vector_field_source(gpu.SOURCE_GIVEN); tr.set_jacobian_field_source(gpu.SOURCE_GIVEN)
    tr.initialize()
    W, H = noisy_woven["dims"]
    with pytest.raises(gpu.FtkxError) as e:
        tr.push_field_data_snapshot(np.zeros((H, W)), np.zeros((H, W, 2)), np.zeros((H, W, 2, 2)))
    assert e.value.code == gpu._lib.E_UNSUPPORTED
    tr.close()


def by_tag_points(points):
    recs, o, ts = points
    k = np.argsort(recs["tag"], kind="stable")
    return np.ascontiguousarray(recs[k]).tobytes(), o[k].tolist(), ts[k].tolist()


def test_two_slab_ranks_add_the_single_trackers_noise(gpu, noisy_woven):
    """two trackers, one per rank and thread, over the in-process hub on one device: each pushes the raw snapshots of its slab under their
    own timesteps, the upper rank's first slice reaches the lower one adjusted already (slab.cpp sets the adjustment aside around that
    push) -- the points and curves of ONE tracker"""
    import threading
    from ftk_amd import tslab, _lib
    L = _lib.load()
    dims, raw, world = noisy_woven["dims"], noisy_woven["raw"], 2
    nt = len(raw)
    hub = L.ftkx_slab_hub_create(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            tr = tracker_of(gpu, dims, adjust=(SIGMA, SEED, CLAMP))
            tr.initialize()
            tr.set_slab_hub(hub, r, nt)
            t0, t1 = tslab.slab_range(nt, world, r)
            for k, t in enumerate(range(t0, t1)):
                tr.push_scalar_field_snapshot(raw[t])
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
    exp = noisy_woven["exp"]
    points, curves, loop = out[0]
    assert by_tag_points(points) == by_tag_points(exp[5])
    assert sorted(zip(map(tuple, curves), loop)) == sorted(zip(map(tuple, exp[3]), exp[4]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    import torch
    E, U = gpu._lib.E_INVALID, gpu._lib.E_UNSUPPORTED
    ctx = gpu.Context(2)
    L, h = ctx._L, ctx._h
    for sigma in (-1.0, float("nan"), float("inf")):
        assert L.ftkx_set_perturbation(h, sigma, 1) == E
    assert L.ftkx_set_clamp(h, 1, float("nan"), 1.0) == E and L.ftkx_set_clamp(h, 1, 0.0, float("nan")) == E
    assert L.ftkx_set_clamp(h, 1, 1.0, -1.0) == 0 and L.ftkx_set_clamp(h, 1, -float("inf"), float("inf")) == 0      # lo > hi and infinite bounds are legal
    assert L.ftkx_set_clamp(h, 0, float("nan"), float("nan")) == 0                                                  # off: the bounds are not looked at
    assert ctx.adjust_counts() == (0, 0, 0)
    # the bare kernel's arguments
    s = torch.zeros(64, dtype=torch.float64, device="cuda"); d = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, q = s.data_ptr(), d.data_ptr()
    assert L.ftkx_adjust(h, None, 8, 1.0, 1, 0, 0, 0.0, 0.0, q) == E and L.ftkx_adjust(h, p, 8, 1.0, 1, 0, 0, 0.0, 0.0, None) == E
    assert L.ftkx_adjust(h, p, 0, 1.0, 1, 0, 0, 0.0, 0.0, q) == E
    assert L.ftkx_adjust(h, p, 8, 0.0, 1, 0, 0, 0.0, 0.0, q) == E                                                   # nothing asked for
    assert L.ftkx_adjust(h, p, 8, -1.0, 1, 0, 0, 0.0, 0.0, q) == E and L.ftkx_adjust(h, p, 8, 0.0, 1, 0, 1, float("nan"), 0.0, q) == E
    assert L.ftkx_adjust(h, p + 4, 8, 1.0, 1, 0, 0, 0.0, 0.0, q) == E and L.ftkx_adjust_f32(h, p + 2, 8, 1.0, 1, 0, 0, 0.0, 0.0, q) == E          # misaligned
    assert L.ftkx_adjust(h, p + 8, 8, 1.0, 1, 0, 0, 0.0, 0.0, p) == E                                               # overlapping, not the same array
    assert L.ftkx_adjust(h, p, 8, 1.0, 1, 0, 0, 0.0, 0.0, p) == 0 and L.ftkx_adjust(h, p, 8, 1.0, 1, 0, 0, 0.0, 0.0, p + 64) == 0
    ms = (C.c_double * 2)()
    assert L.ftkx_debug_adjust_relaunch(h, p, 0, 8, 1.0, 1, 0, 0, 0.0, 0.0, q, 0, ms) == E and L.ftkx_debug_adjust_relaunch(h, p, 0, 8, 1.0, 1, 0, 0, 0.0, 0.0, q, 2, None) == E
    assert L.ftkx_debug_adjust_relaunch(h, p, 0, 8, 1.0, 1, 0, 1, -1.0, 1.0, q, 2, ms) == 0 and ms[0] > 0 and ms[1] > 0
    ctx.close()
    # J (or S) beside V while either setting is on
    mesh = Mesh(gpu, (16, 12), True)
    V, J, S = np.zeros((12, 16, 2)), np.zeros((12, 16, 2, 2)), np.zeros((12, 16))
    for setting in ("perturbation", "clamp"):
        mesh.ctx.set_perturbation(1.0 if setting == "perturbation" else 0.0, 3)
        mesh.ctx.set_clamp(*((0.0, 1.0) if setting == "clamp" else (None, None)))
        for kw in (dict(J=J), dict(S=S), dict(J=J, S=S)):
            with pytest.raises(gpu.FtkxError) as e:
                mesh.ctx.push_slice(0, V, **kw)
            assert e.value.code == U, (setting, sorted(kw))
        mesh.ctx.push_slice(0, V)
    mesh.ctx.set_perturbation(0.0, 0); mesh.ctx.set_clamp()
    mesh.ctx.push_slice(1, V, J=J, S=S)
    mesh.close()
    # set while a series pass is open, or sweeps are pending
    ctx = scalar_context(gpu, (32, 32))
    a = CC.random_input((32, 32), 8)
    ctx.push_scalar_slice(0, a); ctx.push_scalar_slice(1, a)
    ctx.sweep_series_submit([0, 1], [gpu.SCOPE_BOTH, gpu.SCOPE_ORDINAL])
    assert L.ftkx_set_perturbation(ctx._h, 1.0, 1) == E and L.ftkx_set_clamp(ctx._h, 1, 0.0, 1.0) == E
    ctx.sweep_series_abort()
    assert L.ftkx_set_perturbation(ctx._h, 1.0, 1) == 0 and L.ftkx_set_clamp(ctx._h, 1, 0.0, 1.0) == 0
    assert L.ftkx_sweep_enqueue(ctx._h, 0, gpu.SCOPE_ORDINAL, 256) == 0
    assert L.ftkx_set_perturbation(ctx._h, 0.0, 1) == E and L.ftkx_set_clamp(ctx._h, 0, 0.0, 0.0) == E
    assert L.ftkx_sweep_cancel(ctx._h) == 0
    assert L.ftkx_set_perturbation(ctx._h, 0.0, 1) == 0
    ctx.close()
