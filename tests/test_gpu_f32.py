"""Float32 snapshots on the GPU (ftk_amd/csrc/widen_kernels.hip, widen_steps.hpp; the float-source convolution of conv_kernels.hip): the
floats cross PCIe at 4 bytes per value and are widened on the device, in front of everything else.  Widening is exact, so there is no
tolerance anywhere in this file: pushing a float32 array x gives, byte for byte, what pushing x.astype(float64) gives -- through the plain
push, with spatial and temporal smoothing, mixed with FP64 pushes, and through the tracker -- and that in turn is the oracle's answer for
the widened arrays."""
import ctypes as C

import numpy as np
import pytest

import conv_cases as CC
from common import assert_records_equal

pytestmark = pytest.mark.gpu

GRID = 2048 * 256 * 4        # elements one round of the widen kernel's capped grid takes (widen_steps.hpp: kWidenMaxBlocks * kWidenThreads * kWidenGroup)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def wide(a):
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)


# ---- 1. the kernel against numpy ---------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0x00000000, 0x80000000,                # +-0
                    0x7f800000, 0xff800000,                # +-inf
                    0x7f7fffff, 0xff7fffff,                # the largest normal
                    0x00800000, 0x80800000,                # the smallest normal
                    0x00000001, 0x80000001, 0x007fffff, 0x00400000, 0x80000123,   # subnormals, the smallest and the largest among them
                    0x7fc00000, 0xffc00000], dtype=np.uint32)                     # quiet NaNs of both signs


def random_normals(count):
    """float32 bit patterns: either sign, every exponent of a normal number, any mantissa"""
    rng = np.random.default_rng(count)
    bits = (rng.integers(0, 2, size=count, dtype=np.uint32) << 31) | (rng.integers(1, 255, size=count, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, size=count, dtype=np.uint32)
    return bits.astype(np.uint32)


def float_values(normals, seed):
    """random normals over the whole exponent range, the special values at the front and (where there is room) at the back, so that they
    meet the head, the 16-byte body and the tail"""
    bits, count = normals.copy(), len(normals)
    sp = np.roll(SPECIAL, seed)
    k = min(count, len(sp))
    bits[:k] = sp[:k]
    if count >= 2 * len(sp):
        bits[-len(sp):] = sp[::-1]
    return bits.view(np.float32)


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 255, 256, 257, GRID - 1, GRID, GRID + 1])
def test_widen_against_numpy(gpu, count):
    """ftkx_widen_f32 == astype(float64) as 64-bit integers (a NaN: is NaN, same sign), for sources 0..3 floats and destinations 0..1
    doubles behind a 16-byte border; the canaries on both sides of the destination stay.  This is what settles that the conversion
    instruction may be used: subnormals come out as the exact normal doubles"""
    import torch
    ctx = gpu.Context(2)
    pad = 4                                                   # doubles in front of the destination: the 16-byte border is kept
    seen_nan = seen_subnormal = False
    normals = random_normals(count)                           # (made once per count; the special values move with the offsets)
    for src_off in range(4):
        for dst_off in range(2):
            x = float_values(normals, 3 * src_off + 2 * dst_off + 1)       # (count 1: a NaN, subnormals, a normal, an infinity in turn)
            src = torch.zeros(count + 8, dtype=torch.float32, device="cuda")
            src[src_off:src_off + count] = torch.from_numpy(x.copy()).cuda()
            dst = torch.full((count + 2 * pad + 2,), 777.0, dtype=torch.float64, device="cuda")
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            ctx.widen_f32(src.data_ptr() + 4 * src_off, count, dst.data_ptr() + 8 * (pad + dst_off))
            got = dst.cpu().numpy()
            lo = pad + dst_off
            assert np.all(got[:lo] == 777.0) and np.all(got[lo + count:] == 777.0), (count, src_off, dst_off, "a canary was written")
            assert np.array_equal(src[src_off:src_off + count].cpu().numpy().view(np.uint32), x.view(np.uint32)), "the source was written"
            out, exp = got[lo:lo + count], x.astype(np.float64)
            nan = np.isnan(exp)
            seen_nan |= bool(nan.any()); seen_subnormal |= bool(((np.abs(x) > 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any())
            assert np.array_equal(np.isnan(out), nan) and np.array_equal(np.signbit(out[nan]), np.signbit(exp[nan]))
            assert np.array_equal(out.view(np.uint64)[~nan], exp.view(np.uint64)[~nan]), (count, src_off, dst_off)
    assert seen_nan and seen_subnormal
    ctx.close()


# ---- the push path -----------------------------------------------------------------------------------------------------------------------------
def scalar_context(gpu, dims):
    nd = len(dims)
    dom = ([2] * nd, [d - 3 for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
    return ctx


def vector_context(gpu, dims):
    nd = len(dims)
    dom = ([1] * nd, [d - 2 for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=0, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
    return ctx


def as_fixture(recs):
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = recs["aux"] & 1
    out["timestep"] = recs["aux"] >> 1
    return out


def same_records(a, b):
    return len(a) == len(b) and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def handed(a, on_device):
    """the array as the caller hands it over (a host array of its own, or a device tensor) and a copy to hold it to"""
    import torch
    if on_device:
        x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()
        return x, x.clone()
    x = np.ascontiguousarray(a).copy()
    return x, x.copy()


def unchanged_then_overwritten(x, before):
    """the pushed array is as it was; then it is overwritten at once -- the context owns what it needs"""
    import torch
    if hasattr(x, "data_ptr"):
        assert torch.equal(x.view(torch.int32 if x.element_size() == 4 else torch.int64), before.view(torch.int32 if x.element_size() == 4 else torch.int64)), "a pushed tensor was written"
        x.fill_(777.0)
        torch.cuda.synchronize()
    else:
        assert x.tobytes() == before.tobytes(), "a pushed array was written"
        x[...] = 777.0


def sweep_all(gpu, ctx, nt):
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    recs, factors, _ = ctx.sweep_series(range(nt), scopes)
    return recs, [int(f) for f in factors]


def scalar_series(gpu, ctx, slices, on_device=0):
    """pushes the slices -- each unchanged by the push and overwritten right after it, before the sweep -- and sweeps every step in one pass"""
    for t, a in enumerate(slices):
        x, before = handed(a, on_device)
        ctx.push_scalar_slice(t, x, on_device=on_device if on_device else None)
        unchanged_then_overwritten(x, before)
    return sweep_all(gpu, ctx, len(slices))


@pytest.fixture(scope="module")
def woven32(gpu, oracle):
    """the noisy woven series of tests/golden/conv/ rounded to float32: what the FP64 push of the widened slices gives, with and without
    smoothing, and the oracle's records -- computed once"""
    s = CC.series()
    dims = [int(d) for d in s["dims"]]
    x32 = [np.ascontiguousarray(a, dtype=np.float32) for a in s["raw"]]
    x64 = [wide(a) for a in x32]
    out = dict(dims=dims, x32=x32, x64=x64, s=s)
    ctx = scalar_context(gpu, dims)
    out["fp64"] = scalar_series(gpu, ctx, x64)
    assert ctx.f32_counts() == (0, 0)
    ctx.close()
    ref, rf, _ = oracle.track(x64, 2, 1, tag_mode=oracle.TAG_REFERENCE)
    out["oracle"] = (ref, [int(f) for f in rf])
    # the unrounded slices give other records: a push that read the wrong array is seen
    ctx = scalar_context(gpu, dims)
    out["unrounded"] = scalar_series(gpu, ctx, list(s["raw"]))
    ctx.close()
    return out


def bumps(dims=(19, 17, 13), DT=3, seed=1):
    """a sum of four moving Gaussian bumps, rounded to float32 (the oracle finds 33 critical points in this one)"""
    rng = np.random.default_rng(seed)
    nb = 4
    c = rng.uniform(3, [d - 4 for d in dims], size=(nb, 3)); v = rng.uniform(-0.6, 0.6, size=(nb, 3))
    a = rng.uniform(0.5, 1.5, size=nb) * rng.choice([-1, 1], size=nb); sg = rng.uniform(2.0, 3.5, size=nb)
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    out = []
    for k in range(DT):
        S = np.zeros(x.shape)
        for b in range(nb):
            cx, cy, cz = c[b] + k * v[b]
            S += a[b] * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * sg[b] ** 2))
        out.append(S.astype(np.float32))
    return out


BUMP_DIMS = (19, 17, 13)


# ---- 2. push against push, 2D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1, 2])
def test_push_2d(gpu, woven32, on_device):
    exp_recs, exp_factors = woven32["fp64"]
    assert len(exp_recs) > 0 and not same_records(exp_recs, woven32["unrounded"][0])
    ctx = scalar_context(gpu, woven32["dims"])
    recs, factors = scalar_series(gpu, ctx, woven32["x32"], on_device)
    assert len(recs) > 0
    assert factors == exp_factors == woven32["oracle"][1]
    assert same_records(recs, exp_recs)
    assert_records_equal(as_fixture(recs), woven32["oracle"][0], coord_tol=0.0, what=f"float32 push, on_device {on_device}")
    assert ctx.f32_counts() == (8, 0)
    ctx.close()


# ---- 3. the same in 3D, and vector slices ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bumps32(gpu, oracle):
    x32 = bumps()
    x64 = [wide(a) for a in x32]
    ref, rf, _ = oracle.track(x64, 3, 1, tag_mode=oracle.TAG_REFERENCE)
    assert len(ref) > 0
    ctx = scalar_context(gpu, BUMP_DIMS)
    fp64 = scalar_series(gpu, ctx, x64)
    ctx.close()
    return dict(x32=x32, x64=x64, oracle=(ref, [int(f) for f in rf]), fp64=fp64)


@pytest.mark.parametrize("on_device", [0, 1, 2])
def test_push_3d(gpu, bumps32, on_device):
    exp_recs, exp_factors = bumps32["fp64"]
    ctx = scalar_context(gpu, BUMP_DIMS)
    recs, factors = scalar_series(gpu, ctx, bumps32["x32"], on_device)
    assert len(recs) > 0
    assert factors == exp_factors == bumps32["oracle"][1]
    assert same_records(recs, exp_recs)
    assert_records_equal(as_fixture(recs), bumps32["oracle"][0], coord_tol=0.0, what=f"float32 push 3D, on_device {on_device}")
    assert ctx.f32_counts() == (3, 0)
    ctx.close()


def vector_series(gpu, ctx, V, J=None, S=None, on_device=0):
    for t in range(len(V)):
        arrays = [handed(a[t], on_device) if a is not None else (None, None) for a in (V, J, S)]
        ctx.push_slice(t, arrays[0][0], arrays[1][0], arrays[2][0])
        for x, before in arrays:
            if x is not None:
                unchanged_then_overwritten(x, before)
    return sweep_all(gpu, ctx, len(V))


@pytest.mark.parametrize("on_device", [0, 1])
def test_vector_push_2d(gpu, oracle, on_device):
    """ftkx_push_slice_f32 with V alone and with V + J + S (J: the Jacobian the oracle derives from the widened V, rounded; S: any scalar)"""
    import torch
    from ftk_amd import synthetic
    dims, DT = (33, 29), 3
    V32 = [synthetic.double_gyre(dims, k, torch, "cpu").numpy().astype(np.float32) for k in range(DT)]
    V64 = [wide(a) for a in V32]
    J32 = [oracle.jacobian2D(v, 0).astype(np.float32) for v in V64]
    S32 = [np.hypot(v[..., 0], v[..., 1]).astype(np.float32) for v in V64]
    ref, rf, _ = oracle.track(V64, 2, 2, tag_mode=oracle.TAG_REFERENCE)
    assert len(ref) > 0
    for J, S in ((None, None), (J32, S32)):
        A = vector_context(gpu, dims)
        exp_recs, exp_factors = vector_series(gpu, A, V64, None if J is None else [wide(a) for a in J], None if S is None else [wide(a) for a in S])
        A.close()
        B = vector_context(gpu, dims)
        recs, factors = vector_series(gpu, B, V32, J, S, on_device)
        assert B.f32_counts() == (DT * (1 if J is None else 3), 0)
        B.close()
        assert len(recs) > 0 and factors == exp_factors == [int(f) for f in rf]
        assert same_records(recs, exp_recs)
        if J is None:
            assert_records_equal(as_fixture(recs), ref, coord_tol=0.0, what="float32 vector push")
        else:      # (which simplices are hit depends on V alone)
            assert np.array_equal(np.sort(recs["tag"]), np.sort(ref["tag"]))


# ---- 4. spatial smoothing: one kernel from the floats to the smoothed slice --------------------------------------------------------------------
@pytest.mark.parametrize("ksize", [3, 5])
def test_smoothed_push_2d(gpu, oracle, woven32, ksize):
    sigma = 1.0
    A = scalar_context(gpu, woven32["dims"])
    A.set_spatial_smoothing(sigma, ksize)
    exp_recs, exp_factors = scalar_series(gpu, A, woven32["x64"])
    A.close()
    w = gpu.gaussian_kernel(2, sigma, ksize)
    ref, rf, _ = oracle.track([CC.conv(a, w) for a in woven32["x64"]], 2, 1, tag_mode=oracle.TAG_REFERENCE)
    assert len(exp_recs) > 0 and not same_records(exp_recs, woven32["fp64"][0])
    for on_device in (0, 1, 2):
        B = scalar_context(gpu, woven32["dims"])
        B.set_spatial_smoothing(sigma, ksize)
        recs, factors = scalar_series(gpu, B, woven32["x32"], on_device)
        assert B.f32_counts() == (0, 8)
        B.close()
        assert factors == exp_factors == [int(f) for f in rf]
        assert same_records(recs, exp_recs), (ksize, on_device)
        assert_records_equal(as_fixture(recs), ref, coord_tol=0.0, what=f"float32 smoothed push, ksize {ksize}, on_device {on_device}")


def test_smoothed_push_3d(gpu, bumps32):
    A = scalar_context(gpu, BUMP_DIMS)
    A.set_spatial_smoothing(1.0, 3)
    exp_recs, exp_factors = scalar_series(gpu, A, bumps32["x64"])
    A.close()
    assert len(exp_recs) > 0
    for on_device in (0, 1, 2):
        B = scalar_context(gpu, BUMP_DIMS)
        B.set_spatial_smoothing(1.0, 3)
        recs, factors = scalar_series(gpu, B, bumps32["x32"], on_device)
        assert B.f32_counts() == (0, 3)
        B.close()
        assert factors == exp_factors and same_records(recs, exp_recs), on_device


def device_conv(ctx, a, w, f32):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.full(a.shape, 777.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dims = list(reversed(a.shape))
    if a.ndim == 2:
        ctx.conv2D(src.data_ptr(), dims[0], dims[1], w, w.shape[0], out.data_ptr(), f32=f32)
    else:
        ctx.conv3D(src.data_ptr(), dims[0], dims[1], dims[2], w, w.shape[0], out.data_ptr(), f32=f32)
    return out.cpu().numpy()


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("ksize", CC.KSIZES)
def test_conv_f32_border_shapes(gpu, nd, ksize):
    """ftkx_conv2D_f32 / 3D_f32 == ftkx_conv2D / 3D on the widened array, as bytes, on either side of every tile edge"""
    ctx = gpu.Context(nd)
    w = gpu.gaussian_kernel(nd, 0.75 + 0.25 * ksize, ksize)
    for shape in (CC.SHAPES_2D if nd == 2 else CC.SHAPES_3D):
        a32 = CC.shape_input(shape, ksize).astype(np.float32)
        assert CC.same_bits(device_conv(ctx, a32, w, True), device_conv(ctx, wide(a32), w, False)), (shape, ksize)
    ctx.close()


# ---- 5. temporal smoothing -------------------------------------------------------------------------------------------------------------------
def filtered(gpu, dims, slices, K, spatial, on_device):
    """the series through ftkx_temporal_push(_f32) and the flush -> (the emitted timesteps, records, factors)"""
    ctx = scalar_context(gpu, dims)
    if spatial:
        ctx.set_spatial_smoothing(*spatial)
    ctx.set_temporal_smoothing(1.0, K, 0)
    emitted = []
    for a in slices:
        x, before = handed(a, on_device)
        t = ctx.temporal_push(x, on_device=on_device if on_device else None)
        unchanged_then_overwritten(x, before)
        if t >= 0:
            emitted.append(t)
    while True:
        t = ctx.temporal_flush()
        if t < 0:
            break
        emitted.append(t)
    recs, factors = sweep_all(gpu, ctx, len(emitted))
    counts = ctx.f32_counts()
    ctx.close()
    return emitted, recs, factors, counts


@pytest.mark.parametrize("K,spatial", [(5, None), (3, (1.0, 3))])
def test_temporal_push(gpu, woven32, K, spatial):
    exp = filtered(gpu, woven32["dims"], woven32["x64"], K, spatial, 0)
    assert exp[0] == list(range(8)) and len(exp[1]) > 0 and exp[3] == (0, 0)
    for on_device in (0, 1):
        got = filtered(gpu, woven32["dims"], woven32["x32"], K, spatial, on_device)
        assert got[0] == exp[0] and got[2] == exp[2] and same_records(got[1], exp[1]), (K, spatial, on_device)
        assert got[3] == ((0, 8) if spatial else (8, 0))


# ---- 6. mixing ---------------------------------------------------------------------------------------------------------------------------------
def test_float32_and_float64_pushes_alternate(gpu, woven32):
    ctx = scalar_context(gpu, woven32["dims"])
    for t in range(8):
        ctx.push_scalar_slice(t, woven32["x32"][t] if t % 2 == 0 else woven32["x64"][t])
    recs, factors = sweep_all(gpu, ctx, 8)
    assert factors == woven32["fp64"][1] and same_records(recs, woven32["fp64"][0])
    assert ctx.f32_counts() == (4, 0)
    ctx.close()


def test_staging_block_over_meshes_of_rising_and_falling_size(gpu, woven32, bumps32):
    """one context's worth of float32 staging is asked for more, then fewer, then more bytes again, in 2D and in 3D; every series gives
    the records of its FP64 push, and the contexts are destroyed clean"""
    rng = np.random.default_rng(5)
    small32 = [rng.standard_normal((9, 11)).astype(np.float32) for _ in range(2)]
    A = scalar_context(gpu, (11, 9))
    small_exp = scalar_series(gpu, A, [wide(a) for a in small32])
    A.close()
    ctx = gpu.Context(2)
    for dims, x32, exp in (((11, 9), small32, small_exp), (woven32["dims"], woven32["x32"], woven32["fp64"]), ((11, 9), small32, small_exp),
                           (woven32["dims"], woven32["x32"], woven32["fp64"])):
        dom = ([2, 2], [d - 3 for d in dims])
        ctx.set_mesh(dom, dom, ([0, 0], list(dims)))
        ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
        recs, factors = scalar_series(gpu, ctx, x32)
        assert factors == exp[1] and same_records(recs, exp[0]), dims
        for t in range(len(x32)):
            ctx.drop_slice(t)
    assert ctx.f32_counts() == (2 + 8 + 2 + 8, 0)
    ctx.close()
    ctx = gpu.Context(3)
    for dims, x32 in (((9, 8, 7), [a[:7, :8, :9] for a in bumps32["x32"]]), (BUMP_DIMS, bumps32["x32"]), ((9, 8, 7), [a[:7, :8, :9] for a in bumps32["x32"]])):
        dom = ([2] * 3, [d - 3 for d in dims])
        ctx.set_mesh(dom, dom, ([0] * 3, list(dims)))
        ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_REFERENCE)
        recs, factors = scalar_series(gpu, ctx, x32)
        A = scalar_context(gpu, dims)
        exp = scalar_series(gpu, A, [wide(a) for a in x32])
        A.close()
        assert factors == exp[1] and same_records(recs, exp[0]), dims
        for t in range(len(x32)):
            ctx.drop_slice(t)
    ctx.close()


# ---- 7. the tracker ----------------------------------------------------------------------------------------------------------------------------
def tracked(gpu, slices, dims, device=False, device_ids=None):
    import torch
    tr = gpu.CriticalPointTracker2DRegular(device_ids=device_ids)
    try:
        tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
        tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
        tr.set_domain([2, 2], [d - 3 for d in dims]); tr.set_array_domain([0, 0], list(dims))
        tr.initialize()
        for k, a in enumerate(slices):
            if device:
                a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                torch.cuda.synchronize()
            tr.push_scalar_field_snapshot(a)
            if device:
                a.fill_(777.0)                 # (a float32 snapshot is read before the push returns)
                torch.cuda.synchronize()
            if k:
                tr.advance_timestep()
        tr.update_timestep()
        recs, o, ts = tr.get_critical_points()
        tr.finalize()
        curves, loop = tr.get_traced_critical_points()
        return recs, o, ts, [c.tolist() for c in curves], loop.tolist()
    finally:
        tr.close()


def test_tracker_takes_float32(gpu, woven32):
    exp = tracked(gpu, woven32["x64"], woven32["dims"])
    assert len(exp[0]) > 0 and len(exp[3]) > 0
    for device in (False, True):
        got = tracked(gpu, woven32["x32"], woven32["dims"], device=device)
        assert same_records(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
        assert got[3] == exp[3] and got[4] == exp[4]
    with pytest.raises(gpu.FtkxError) as e:
        tracked(gpu, woven32["x32"], woven32["dims"], device_ids=[0, 0])
    assert e.value.code == gpu._lib.E_UNSUPPORTED


def test_element_types_of_tensors(gpu, woven32):
    """a float32 torch tensor is pushed as it is (it used to raise TypeError); float16 still raises; an int32 tensor is passed on as before"""
    import torch
    ctx = scalar_context(gpu, woven32["dims"])
    ctx.push_scalar_slice(0, torch.from_numpy(woven32["x32"][0]))                    # a host tensor
    ctx.push_scalar_slice(1, torch.from_numpy(woven32["x32"][1]).cuda())
    assert ctx.f32_counts() == (2, 0)
    with pytest.raises(TypeError):
        ctx.push_scalar_slice(2, torch.zeros(tuple(reversed(woven32["dims"])), dtype=torch.float16))
    assert gpu._ptr(torch.zeros(4, dtype=torch.int32))[3] is False and gpu._ptr(np.zeros(4, dtype=np.int32))[3] is False
    with pytest.raises(TypeError):
        ctx.push_slice(3, np.zeros((4, 4, 2), dtype=np.float32), np.zeros((4, 4, 2, 2)))      # one push, two element types
    ctx.close()


# ---- 8. argument errors: the codes of the FP64 entries -----------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    import torch
    L = gpu._lib.load()
    E, U = gpu._lib.E_INVALID, gpu._lib.E_UNSUPPORTED
    a32 = np.zeros((12, 16), dtype=np.float32); a64 = np.zeros((12, 16)); v32 = np.zeros((12, 16, 2), dtype=np.float32); v64 = np.zeros((12, 16, 2))
    t = C.c_int(0)
    ctx = gpu.Context(2)
    h = ctx._h
    # before ftkx_set_mesh
    assert L.ftkx_push_scalar_slice_f32(h, 0, a32.ctypes.data, 0) == L.ftkx_push_scalar_slice(h, 0, a64.ctypes.data, 0) == E
    ctx.set_mesh(([1, 1], [14, 10]), ([1, 1], [14, 10]), ([0, 0], [16, 12]))
    ctx.set_options(jacobian_symmetric=0, derive_jacobian=1)
    assert L.ftkx_push_scalar_slice_f32(None, 0, a32.ctypes.data, 0) == L.ftkx_push_scalar_slice(None, 0, a64.ctypes.data, 0) == E
    assert L.ftkx_push_scalar_slice_f32(h, 0, None, 0) == L.ftkx_push_scalar_slice(h, 0, None, 0) == E
    assert L.ftkx_push_slice_f32(h, 0, None, None, a32.ctypes.data, 0) == L.ftkx_push_slice(h, 0, None, None, a64.ctypes.data, 0) == E
    assert L.ftkx_push_scalar_slice_f32(h, 0, a32.ctypes.data, 3) == L.ftkx_push_scalar_slice(h, 0, a64.ctypes.data, 3) == E
    assert L.ftkx_push_scalar_slice_f32(h, -1, a32.ctypes.data, 0) == L.ftkx_push_scalar_slice(h, -1, a64.ctypes.data, 0) == E
    assert L.ftkx_temporal_push_f32(h, a32.ctypes.data, 0, 0, C.byref(t)) == L.ftkx_temporal_push(h, a64.ctypes.data, 0, 0, C.byref(t)) == E      # no filter set
    ctx.set_spatial_smoothing(1.0, 3)
    assert L.ftkx_push_slice_f32(h, 0, v32.ctypes.data, None, None, 0) == L.ftkx_push_slice(h, 0, v64.ctypes.data, None, None, 0) == U
    ctx.set_temporal_smoothing(1.0, 3, 0)
    assert L.ftkx_temporal_push_f32(h, v32.ctypes.data, 1, 0, C.byref(t)) == L.ftkx_temporal_push(h, v64.ctypes.data, 1, 0, C.byref(t)) == U
    assert L.ftkx_temporal_push_f32(h, None, 0, 0, C.byref(t)) == L.ftkx_temporal_push(h, None, 0, 0, C.byref(t)) == E
    assert L.ftkx_temporal_push_f32(h, a32.ctypes.data, 0, 0, None) == E
    ctx.set_temporal_smoothing(0.0, 0, 0)
    ctx.set_spatial_smoothing(0.0, 0)
    # the stand-alone entries
    s = torch.zeros(64, dtype=torch.float32, device="cuda"); d = torch.zeros(64, dtype=torch.float64, device="cuda")
    w = np.full(81, 1.0 / 81)
    assert L.ftkx_widen_f32(h, None, 8, d.data_ptr()) == E and L.ftkx_widen_f32(h, s.data_ptr(), 8, None) == E
    assert L.ftkx_widen_f32(h, s.data_ptr(), 0, d.data_ptr()) == E
    assert L.ftkx_widen_f32(h, s.data_ptr() + 2, 8, d.data_ptr()) == E and L.ftkx_widen_f32(h, s.data_ptr(), 8, d.data_ptr() + 4) == E      # misaligned
    assert L.ftkx_widen_f32(h, d.data_ptr() + 16, 8, d.data_ptr()) == E                                                                  # overlapping
    assert L.ftkx_conv2D_f32(h, s.data_ptr(), 8, 8, w.ctypes.data, 4, d.data_ptr()) == L.ftkx_conv2D(h, d.data_ptr(), 8, 4, w.ctypes.data, 4, d.data_ptr() + 256) == E
    assert L.ftkx_conv2D_f32(h, s.data_ptr(), 0, 8, w.ctypes.data, 3, d.data_ptr()) == E and L.ftkx_conv2D_f32(h, None, 8, 8, w.ctypes.data, 3, d.data_ptr()) == E
    ms = (C.c_double * 2)()
    assert L.ftkx_debug_widen_relaunch(h, s.data_ptr(), 8, d.data_ptr(), 0, ms) == E
    assert L.ftkx_debug_f32_counts(None, None, None) == E
    ctx.close()
