"""Temporal Gaussian smoothing on the GPU (ftk_amd/csrc/temporal_kernels.hip, temporal_steps.hpp): ftkx_temporal_push / _flush against the
reference's own outputs (tests/golden/temporal/) -- the emitted timesteps, and the resident slices read back through the patches the halo
exchange uses -- ftkx_temporal_combine against the numpy restatement of tests/temporal_cases.py, all as uint64; then the filter behind
the spatial smoothing, and in front of the tracker: a tracker that filters the raw series must give what a plain tracker gives that is
handed the reference's smoothed arrays."""
import numpy as np
import pytest

import conv_cases as CC
import temporal_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- a context over a fixture's mesh, and its resident slices read back -------------------------------------------------------------------
class Mesh:
    def __init__(self, gpu, dims, vector):
        """dims: the mesh extents, x first; scalar meshes keep two vertices to every border (the gradient of the gradient), vector ones one"""
        self.gpu, self.dims, self.vector = gpu, [int(d) for d in dims], vector
        nd = self.nd = len(dims)
        self.core = ([1] * nd, [d - 2 for d in self.dims]) if vector else ([2] * nd, [d - 3 for d in self.dims])
        self.ctx = gpu.Context(nd)
        self.ctx.set_mesh(self.core, self.core, ([0] * nd, self.dims))
        if vector:
            self.ctx.set_options(jacobian_symmetric=0, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
        else:
            self.ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)

    def read(self, t):
        """the resident slice t as a host array (x last; a vector slice: components last), put together from the patches around every cell
        of the core: array coordinates corner - 2 .. corner + 3 per axis, clamped (ftkx_gather_patches)"""
        import torch
        nd, dims, ncomp = self.nd, self.dims, (self.nd if self.vector else 1)
        st, sz = self.core
        ncell = int(np.prod(sz))
        cells = torch.arange(ncell, dtype=torch.int64, device="cuda")
        assert self.ctx.patch_doubles() == 6 ** nd * ncomp
        p = self.ctx.gather_patches(t, cells, torch).cpu().numpy().reshape(ncell, 6 ** nd, ncomp)
        lin = np.arange(ncell)
        q = np.arange(6 ** nd)
        at = np.zeros((ncell, 6 ** nd), dtype=np.int64)
        stride = 1
        for a in range(nd):
            corner = st[a] + lin % sz[a]; lin = lin // sz[a]
            x = np.clip(corner[:, None] - 2 + (q % 6)[None, :], 0, dims[a] - 1); q = q // 6
            at += x * stride; stride *= dims[a]
        out = np.full((stride, ncomp), 777.0)
        seen = np.zeros(stride, dtype=bool)
        out[at.ravel()] = p.reshape(-1, ncomp)
        seen[at.ravel()] = True
        assert seen.all(), "the patches do not cover the array"
        shape = tuple(reversed(dims)) + ((ncomp,) if self.vector else ())
        return out.reshape(shape)

    def close(self):
        self.ctx.close()


def mesh_of(gpu, f, vector):
    """(a vector fixture's dims start with its number of components)"""
    dims = [int(d) for d in f["dims"]]
    return Mesh(gpu, dims[1:] if vector else dims, vector)


def run_filter(mesh, raw, on_device, emitted, overwrite=True):
    """pushes the raw arrays, then flushes until the filter says -1; emitted: takes (timestep, slice read back) in order.  A device source
    (on_device 1 / 2) must be unchanged after the push and is overwritten at once: the ring owns a copy"""
    import torch
    ctx = mesh.ctx
    for a in raw:
        if on_device:
            x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            before = x.clone()
            torch.cuda.synchronize()
            t = ctx.temporal_push(x, is_vector=mesh.vector, on_device=on_device)
            assert torch.equal(x.view(torch.int64), before.view(torch.int64)), "a pushed tensor was written"
            if overwrite:
                x.fill_(777.0)
                torch.cuda.synchronize()
        else:
            t = ctx.temporal_push(a, is_vector=mesh.vector)
        if t >= 0:
            emitted.append((t, mesh.read(t)))
    while True:
        t = ctx.temporal_flush()
        if t < 0:
            break
        emitted.append((t, mesh.read(t)))


@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(TC.EXPECTED_OUTPUTS))
def test_fixtures_through_push_and_flush(gpu, name, on_device):
    f = TC.load(name)
    mesh = mesh_of(gpu, f, name == TC.VECTOR)
    t0 = 3
    mesh.ctx.set_temporal_smoothing(float(f["sigma"]), int(f["ksize"]), t0)
    got = []
    run_filter(mesh, list(f["input"]), on_device, got)
    assert [t for t, _ in got] == list(range(t0, t0 + TC.EXPECTED_OUTPUTS[name])), name
    for n, (t, a) in enumerate(got):
        assert np.array_equal(bits(a), bits(f["output"][n])), (name, n)
    # the filter is in its initial state and numbers on from the next unused timestep: the same series again, the slices of the first
    # one still resident
    again = []
    run_filter(mesh, list(f["input"]), on_device, again)
    assert [t for t, _ in again] == list(range(t0 + len(got), t0 + 2 * len(got)))
    for n, (t, a) in enumerate(again):
        assert np.array_equal(bits(a), bits(f["output"][n])), (name, n)
    for t, a in got[:2]:      # (what the second series wrote lies in buffers of its own)
        assert np.array_equal(bits(mesh.read(t)), bits(a))
    mesh.close()


def test_emitted_slices_sweep_like_pushed_ones(gpu):
    """the smoothed slices of the woven series, emitted by the filter, against the same arrays pushed as they are: same records, same factors"""
    s = TC.series()
    DT = int(s["DT"])
    scopes = [gpu.SCOPE_BOTH if t + 1 < DT else gpu.SCOPE_ORDINAL for t in range(DT)]
    A = Mesh(gpu, s["dims"], False)
    for t, a in enumerate(s["smoothed"]):
        A.ctx.push_scalar_slice(t, a)
    exp, exp_f, _ = A.ctx.sweep_series(range(DT), scopes)
    A.close()
    B = Mesh(gpu, s["dims"], False)
    B.ctx.set_temporal_smoothing(float(s["sigma"]), int(s["ksize"]), 0)
    got = []
    run_filter(B, list(s["raw"]), 0, got)
    assert [t for t, _ in got] == list(range(DT))
    assert np.array_equal(bits(np.stack([a for _, a in got])), bits(s["smoothed"]))
    recs, f, _ = B.ctx.sweep_series(range(DT), scopes)
    B.close()
    assert len(exp) > 0 and [int(x) for x in f] == [int(x) for x in exp_f]
    assert np.ascontiguousarray(recs).tobytes() == np.ascontiguousarray(exp).tobytes()


# ---- the bare kernel --------------------------------------------------------------------------------------------------------------------------
GRID_DOUBLES = 2048 * 256 * 2                        # what one round of the capped grid covers at 16 bytes per lane (temporal_steps.hpp)
COUNTS = (1, 2, 3, 255, 256, 257, 31 * 37)
BIG = GRID_DOUBLES + 513                             # odd: the grid-stride loop's second round and the tail meet


def patterns(K):
    """pointer lists: all distinct; the first array repeated (the start of a series); the last repeated (its end); any repeats"""
    H = (K + 1) // 2
    yield list(range(K))
    if K > 1:
        yield [max(0, i - (H - 1)) for i in range(K)]
        yield [min(H - 1, i) for i in range(K)]
        yield [(i * 2) % 3 for i in range(K)]


def device_combine(gpu, ctx, host_arrays, pattern, w, misalign=False):
    import torch
    count = host_arrays[0].size
    pad = 1 if misalign else 0
    dev = [torch.zeros(count + pad, dtype=torch.float64, device="cuda") for _ in host_arrays]
    for d, a in zip(dev, host_arrays):
        d[pad:].copy_(torch.from_numpy(a))
    keep = [d.clone() for d in dev]
    out = torch.full((count + pad + 2,), 777.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.temporal_combine([dev[j].data_ptr() + 8 * pad for j in pattern], w, count, out.data_ptr() + 8 * pad)
    for d, k in zip(dev, keep):
        assert torch.equal(d.view(torch.int64), k.view(torch.int64)), "an input was written"
    o = out.cpu().numpy()
    assert (o[:pad] == 777.0).all() and (o[pad + count:] == 777.0).all(), "a store outside the output"
    return o[pad:pad + count]


@pytest.mark.parametrize("K", TC.KSIZES)
def test_combine_against_the_restatement(gpu, K):
    ctx = gpu.Context(2)
    w = TC.gaussian_weights(0.5 + 0.25 * K, K)
    for count in COUNTS:
        arrays = list(TC.random_input((K, count), 7000 + 10 * K + count % 97))
        for pattern in patterns(K):
            for misalign in (False, True):
                got = device_combine(gpu, ctx, arrays, pattern, w, misalign)
                assert np.array_equal(bits(got), bits(TC.combine([arrays[j] for j in pattern], w))), (K, count, pattern, misalign)
    ctx.close()


@pytest.mark.parametrize("K", TC.KSIZES)
def test_combine_more_than_one_grid_round(gpu, K):
    """a count above one round of the capped grid, odd: all distinct arrays on the 16-byte and on the 8-byte path (there the round is half as
    long), and an edge pattern"""
    ctx = gpu.Context(2)
    w = TC.gaussian_weights(1.0, K)
    arrays = list(TC.random_input((K, BIG), 7100 + K))
    H = (K + 1) // 2
    for pattern, misalign in ((list(range(K)), False), (list(range(K)), True), ([max(0, i - (H - 1)) for i in range(K)], False)):
        got = device_combine(gpu, ctx, arrays, pattern, w, misalign)
        assert np.array_equal(bits(got), bits(TC.combine([arrays[j] for j in pattern], w))), (K, pattern, misalign)
    ctx.close()


def test_combine_inf_and_nan(gpu):
    ctx = gpu.Context(2)
    K, count = 5, 257
    w = TC.gaussian_weights(1.0, K)
    arrays = list(TC.random_input((K, count), 7200))
    arrays[1][100], arrays[2][100] = np.inf, -np.inf      # one element sees Inf - Inf
    arrays[3][101] = np.inf
    arrays[0][256] = -np.inf                              # the tail element
    got = device_combine(gpu, ctx, arrays, list(range(K)), w)
    exp = TC.combine(arrays, w)
    assert np.isnan(exp[100]) and np.isinf(exp[101]) and np.isinf(exp[256]) and TC.same_bits(got, exp)
    arrays = list(TC.random_input((K, count), 7201))
    arrays[4][7] = np.nan
    got = device_combine(gpu, ctx, arrays, [0, 0, 1, 4, 4], w)
    exp = TC.combine([arrays[j] for j in (0, 0, 1, 4, 4)], w)
    assert np.isnan(exp).sum() == 1 and TC.same_bits(got, exp)
    ctx.close()


def test_argument_errors(gpu):
    import ctypes as C
    import torch
    E, U = gpu._lib.E_INVALID, gpu._lib.E_UNSUPPORTED
    a = torch.zeros(64, dtype=torch.float64, device="cuda"); b = torch.zeros(64, dtype=torch.float64, device="cuda")
    ctx = gpu.Context(2)
    L, h = ctx._L, ctx._h
    w = np.full(9, 1.0 / 9)
    ptrs = (C.c_void_p * 9)(*([a.data_ptr()] * 9))
    assert L.ftkx_temporal_combine(h, ptrs, 4, w.ctypes.data, 64, b.data_ptr()) == E
    assert L.ftkx_temporal_combine(h, ptrs, 11, w.ctypes.data, 64, b.data_ptr()) == E
    assert L.ftkx_temporal_combine(h, ptrs, 3, w.ctypes.data, 0, b.data_ptr()) == E
    assert L.ftkx_temporal_combine(h, ptrs, 3, None, 64, b.data_ptr()) == E
    assert L.ftkx_temporal_combine(h, ptrs, 3, w.ctypes.data, 64, a.data_ptr()) == E                  # in place
    assert L.ftkx_temporal_combine(h, ptrs, 3, w.ctypes.data, 32, a.data_ptr() + 8 * 16) == E         # overlapping
    assert L.ftkx_temporal_combine(h, ptrs, 3, w.ctypes.data, 32, a.data_ptr() + 8 * 32) == 0         # side by side
    for sigma, ksize in ((1.0, 4), (1.0, 11), (1.0, -1), (0.0, 3), (float("nan"), 3), (float("inf"), 3)):
        assert L.ftkx_set_temporal_smoothing(h, sigma, ksize, 0) == E
    assert L.ftkx_set_temporal_smoothing(h, 1.0, 3, -1) == E
    t = C.c_int(5)
    x = np.zeros((12, 16))
    assert L.ftkx_temporal_push(h, x.ctypes.data, 0, 0, C.byref(t)) == E and t.value == -1           # the filter is off
    assert L.ftkx_temporal_flush(h, C.byref(t)) == E
    assert L.ftkx_set_temporal_smoothing(h, 1.0, 3, 0) == 0
    assert L.ftkx_temporal_push(h, x.ctypes.data, 0, 0, C.byref(t)) == E                             # no mesh
    ctx.set_mesh(([2, 2], [13, 9]), ([2, 2], [13, 9]), ([0, 0], [16, 12]))
    assert L.ftkx_temporal_push(h, x.ctypes.data, 0, 3, C.byref(t)) == E
    assert L.ftkx_temporal_push(h, None, 0, 0, C.byref(t)) == E
    assert [ctx.temporal_push(x) for _ in range(3)] == [-1, 0, 1]
    v = np.zeros((12, 16, 2))
    with pytest.raises(gpu.FtkxError) as e:                                                          # a vector snapshot in a scalar series
        ctx.temporal_push(v, is_vector=True)
    assert e.value.code == E
    assert ctx.temporal_flush() == 2 and ctx.temporal_flush() == -1
    for t_ in (0, 1, 2):
        ctx.drop_slice(t_)
    # a new series may be of the other kind -- unless spatial smoothing is set
    ctx.set_spatial_smoothing(1.0, 3)
    with pytest.raises(gpu.FtkxError) as e:
        ctx.temporal_push(v, is_vector=True)
    assert e.value.code == U
    ctx.set_spatial_smoothing(0.0, 0)
    assert [ctx.temporal_push(v, is_vector=True) for _ in range(3)] == [-1, 3, 4]
    with pytest.raises(gpu.FtkxError) as e:
        ctx.temporal_push(x)
    assert e.value.code == E
    assert ctx.temporal_flush() == 5
    with pytest.raises(gpu.FtkxError):                                                               # between the first flush and its -1
        ctx.temporal_push(v, is_vector=True)
    ctx.set_temporal_smoothing(0.0, 0)                                                               # off: the ring is released
    ctx.push_slice(7, v)                                                                             # the plain push is as it was
    ctx.close()


# ---- behind the spatial smoothing -------------------------------------------------------------------------------------------------------------
def test_spatial_then_temporal(gpu):
    """the stream's order: every raw snapshot is convolved (the conv fixture's kernel, by ftkx_conv2D) and the filter runs over the results"""
    import torch
    s, sp = TC.series(), CC.series()
    w2 = gpu.gaussian_kernel(2, float(sp["sigma"]), int(sp["ksize"]))
    assert np.array_equal(bits(w2), bits(sp["weights"]))
    mesh = Mesh(gpu, s["dims"], False)
    conv = []
    for a in s["raw"]:
        src = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out = torch.empty_like(src)
        torch.cuda.synchronize()
        mesh.ctx.conv2D(src.data_ptr(), mesh.dims[0], mesh.dims[1], w2, int(sp["ksize"]), out.data_ptr())
        conv.append(out.cpu().numpy())
    assert np.array_equal(bits(conv[0]), bits(CC.conv(s["raw"][0], w2)))
    exp = TC.smooth_series(conv, s["weights"])
    plain = TC.smooth_series(list(s["raw"]), s["weights"])
    assert len(exp) == 12 and not np.array_equal(bits(exp[5]), bits(plain[5]))
    for on_device in (0, 1):
        mesh.ctx.set_spatial_smoothing(float(sp["sigma"]), int(sp["ksize"]))
        mesh.ctx.set_temporal_smoothing(float(s["sigma"]), int(s["ksize"]), 0)
        got = []
        run_filter(mesh, list(s["raw"]), on_device, got)
        assert [t for t, _ in got] == list(range(12))
        assert np.array_equal(bits(np.stack([a for _, a in got])), bits(np.stack(exp))), on_device
    mesh.close()


# ---- the tracker ------------------------------------------------------------------------------------------------------------------------------
def tracker_of(gpu, dims, temporal=None, deferred=False, **kw):
    tr = gpu.CriticalPointTracker2DRegular(**kw)
    tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
    tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
    tr.set_domain([2, 2], [d - 3 for d in dims]); tr.set_array_domain([0, 0], list(dims))
    if temporal:
        tr.set_temporal_smoothing(*temporal)
    return tr


def feed(gpu, tr, slices, filtered, device=False):
    """the reference's loop -- push, advance_timestep() from the second snapshot on, update_timestep() after the last -- where a snapshot is
    whatever the filter emits; -> (factors per step, how many snapshots each push gave)"""
    import torch
    factors, gave = [], []
    n = 0

    def arrived():
        nonlocal n
        if n:
            tr.advance_timestep()
            factors.append(int(tr.get_vector_field_scaling_factor()))
        n += 1

    for a in slices:
        if device:
            a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            torch.cuda.synchronize()
        tr.push_scalar_field_snapshot(a)
        gave.append(tr.snapshots_from_last_push())
        if gave[-1]:
            arrived()
    while filtered and tr.flush_temporal_smoothing():
        arrived()
    tr.update_timestep()
    factors.append(int(tr.get_vector_field_scaling_factor()))
    return factors, gave


def results(tr):
    recs, o, ts = tr.get_critical_points()
    tr.finalize()
    curves, loop = tr.get_traced_critical_points()
    return np.ascontiguousarray(recs).tobytes(), o.tolist(), ts.tolist(), [c.tolist() for c in curves], loop.tolist()


def tracked(gpu, slices, dims, temporal=None, device=False, deferred=False):
    tr = tracker_of(gpu, dims, temporal)
    tr.initialize()
    if deferred:
        tr.set_deferred_collection(True)
    factors, gave = feed(gpu, tr, slices, bool(temporal), device)
    if deferred:
        factors = [int(tr.get_vector_field_scaling_factor())]      # (queued steps: only the last factor is the step's own)
    out = results(tr) + (factors, gave)
    tr.close()
    return out


@pytest.fixture(scope="module")
def woven(gpu):
    s = TC.series()
    dims = [int(d) for d in s["dims"]]
    return dict(s=s, dims=dims, smoothed=tracked(gpu, list(s["smoothed"]), dims), raw=tracked(gpu, list(s["raw"]), dims))


def test_the_noise_matters(woven):
    """(else the tracker tests below would pass with the filter left out)"""
    assert len(woven["smoothed"][0]) > 0 and len(woven["smoothed"][3]) > 0
    assert woven["smoothed"][0] != woven["raw"][0]
    assert woven["smoothed"][6] == [1] * 12


@pytest.mark.parametrize("variant", ["host", "device", "deferred_device"])
def test_tracker_filters_in_front_of_the_sweep(gpu, woven, variant):
    s = woven["s"]
    got = tracked(gpu, list(s["raw"]), woven["dims"], temporal=(float(s["sigma"]), int(s["ksize"])), device=variant != "host", deferred=variant == "deferred_device")
    exp = woven["smoothed"]
    assert got[6] == [0, 0] + [1] * 10                      # ksize 5: the filter answers two pushes late
    assert got[0] == exp[0] and got[1] == exp[1] and got[2] == exp[2], variant
    assert got[3] == exp[3] and got[4] == exp[4], variant
    assert got[5] == (exp[5] if variant != "deferred_device" else exp[5][-1:]), variant


def test_reset_mid_series(gpu, woven):
    """the first five raw snapshots in (three smoothed ones out, two steps swept), reset(), then the whole series: what a fresh tracker gives"""
    s = woven["s"]
    tr = tracker_of(gpu, woven["dims"], temporal=(float(s["sigma"]), int(s["ksize"])))
    tr.initialize()
    for k in range(5):
        tr.push_scalar_field_snapshot(s["raw"][k])
        if tr.snapshots_from_last_push() and k > 2:
            tr.advance_timestep()
    tr.reset()
    factors, gave = feed(gpu, tr, list(s["raw"]), True)
    got = results(tr)
    tr.close()
    exp = woven["smoothed"]
    assert gave == [0, 0] + [1] * 10                      # the ring was emptied: the filter answers two pushes late again
    assert got[:5] == exp[:5]
    # reset() keeps the running resolution (as the reference's does), so a factor after it can only be the fresh tracker's or larger; what
    # was swept before the reset are this series' own first smoothed snapshots, which the running minimum of the fresh tracker takes in
    # as well from its second step on
    assert factors[1:] == exp[5][1:] and factors[0] >= exp[5][0]


def test_snapshots_from_last_push_with_the_filter_switched_off_again(gpu, woven):
    """a push that emitted nothing, then the filter off and initialize(): every plain push gives one snapshot, and says so"""
    s = woven["s"]
    tr = tracker_of(gpu, woven["dims"], temporal=(1.0, 5))
    tr.initialize()
    assert tr.snapshots_from_last_push() == 1
    tr.push_scalar_field_snapshot(s["raw"][0])
    assert tr.snapshots_from_last_push() == 0
    tr.set_temporal_smoothing(0.0, 0)
    tr.initialize()
    tr.push_scalar_field_snapshot(s["smoothed"][0])
    assert tr.snapshots_from_last_push() == 1
    tr.push_scalar_field_snapshot(s["smoothed"][1])
    tr.advance_timestep()
    tr.update_timestep()
    recs, o, ts = tr.get_critical_points()
    assert sorted(set(ts.tolist())) == [0, 1]
    tr.close()


def test_field_data_push_is_refused(gpu, woven):
    tr = tracker_of(gpu, woven["dims"], temporal=(1.0, 5))
    tr.set_vector_field_source(gpu.SOURCE_GIVEN); tr.set_jacobian_field_source(gpu.SOURCE_GIVEN)
    tr.initialize()
    W, H = woven["dims"]
    with pytest.raises(gpu.FtkxError) as e:
        tr.push_field_data_snapshot(np.zeros((H, W)), np.zeros((H, W, 2)), np.zeros((H, W, 2, 2)))
    assert e.value.code == gpu._lib.E_UNSUPPORTED
    tr.close()


def test_slab_and_multi_device_trackers_are_refused(gpu, woven):
    from ftk_amd import _lib
    L = _lib.load()
    U = gpu._lib.E_UNSUPPORTED
    hub = L.ftkx_slab_hub_create(2)
    # the filter set, then slab mode
    tr = tracker_of(gpu, woven["dims"], temporal=(1.0, 5))
    tr.initialize()
    with pytest.raises(gpu.FtkxError) as e:
        tr.set_slab_hub(hub, 0, 12)
    assert e.value.code == U
    tr.close()
    # slab mode, then the filter: initialize() says so
    tr = tracker_of(gpu, woven["dims"])
    tr.initialize()
    tr.set_slab_hub(hub, 0, 12)
    tr.set_temporal_smoothing(1.0, 5)
    with pytest.raises(gpu.FtkxError) as e:
        tr.initialize()
    assert e.value.code == U
    tr.close()
    L.ftkx_slab_hub_destroy(hub)
    tr = tracker_of(gpu, woven["dims"], temporal=(1.0, 5), device_ids=[0, 0])
    with pytest.raises(gpu.FtkxError) as e:
        tr.initialize()
    assert e.value.code == U
    tr.close()
    # and without the filter both are as they were
    tr = tracker_of(gpu, woven["dims"], device_ids=[0, 0])
    tr.initialize()
    tr.close()
