"""Half, bfloat16 and integer snapshots on the GPU (ftk_amd/csrc/narrow_kernels.hip, narrow_steps.hpp; narrow_ingest_plan of ingest_steps.hpp):
the elements cross PCIe at 1, 2 or 4 bytes per value and are widened on the device, in front of everything else.  Every value of every one
of these types is a double, so there is no tolerance anywhere in this file: pushing a narrow array x gives, byte for byte, what pushing
x.astype(float64) gives -- through the plain push, with spatial smoothing, clamp, perturbation and the temporal filter behind it, mixed with
float32 and FP64 pushes, and through the tracker -- and that in turn is the oracle's answer for the widened arrays.  The yardstick for the
kernel is numpy's astype(float64), which tests/test_narrow_golden.py holds to the reference's own from_array."""
import ctypes as C

import numpy as np
import pytest

from common import assert_records_equal
from test_gpu_temporal import Mesh

pytestmark = pytest.mark.gpu

F64, F32, F16, BF16, U8, I8, U16, I16, U32, I32 = range(10)          # FTKX_DTYPE_* (include/ftkx.h)
STORAGE = {F16: np.uint16, BF16: np.uint16, U8: np.uint8, I8: np.int8, U16: np.uint16, I16: np.int16, U32: np.uint32, I32: np.int32}
NARROW = sorted(STORAGE)
COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025)                   # (the host test's; count 0 is refused: test_contract_errors)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def yardstick(dtype, stored):
    """what `stored` (the elements as numpy holds their bits) widens to"""
    with np.errstate(invalid="ignore"):          # (signalling NaNs among the bit patterns)
        if dtype == F16:
            return stored.view(np.float16).astype(np.float64)
        if dtype == BF16:
            return (stored.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return stored.astype(np.float64)


def assert_same(got, exp, what):
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.signbit(got), np.signbit(exp)), what
    assert np.array_equal(got.view(np.uint64)[~nan], exp.view(np.uint64)[~nan]), what


def patterns(dtype, count, seed=0):
    """`count` elements of the type as numpy holds them: for the 8- and 16-bit types ALL their bit patterns in turn, starting anywhere; for
    the 32-bit ones the named values in front of seeded ones"""
    size = np.dtype(STORAGE[dtype]).itemsize
    if size < 4:
        bits = ((np.arange(count, dtype=np.uint64) * (1 if count >= 256 ** size else 2654435761) + seed * 7919) % (256 ** size))
        return bits.astype(np.uint8 if size == 1 else np.uint16).view(STORAGE[dtype])
    named = np.array([0, 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1], dtype=np.uint64)
    bits = np.random.default_rng(100 * dtype + seed).integers(0, 2 ** 32, size=count, dtype=np.uint64)
    bits[:min(count, len(named))] = np.roll(named, seed)[:min(count, len(named))]
    return bits.astype(np.uint32).view(STORAGE[dtype])


def widen_on_device(ctx, dtype, stored, src_off, dst_off, pad=4):
    """ftkx_widen_typed of `stored` lying src_off elements behind a 16-byte border into a destination dst_off doubles behind one, with guard
    values of 777.0 on both sides -> the widened array"""
    import torch
    size, count = stored.dtype.itemsize, len(stored)
    raw = np.zeros((count + 8) * size, dtype=np.uint8)
    raw[src_off * size:(src_off + count) * size] = stored.view(np.uint8)
    src = torch.from_numpy(raw).cuda()
    dst = torch.full((count + 2 * pad + 2,), 777.0, dtype=torch.float64, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.widen_typed(src.data_ptr() + size * src_off, dtype, count, dst.data_ptr() + 8 * (pad + dst_off))
    got = dst.cpu().numpy()
    lo = pad + dst_off
    assert np.all(got[:lo] == 777.0) and np.all(got[lo + count:] == 777.0), (dtype, count, src_off, dst_off, "a guard value was written")
    assert np.array_equal(src.cpu().numpy(), raw), "the source was written"
    return got[lo:lo + count]


# ---- 1. the kernel against numpy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NARROW)
def test_widen_typed_small_counts(gpu, dtype):
    """ftkx_widen_typed == the yardstick as 64-bit integers, for sources 0..3 elements and destinations 0..1 doubles behind their borders
    (both the 4-element body and the element-wise form), guard values on both sides of the destination untouched"""
    ctx = gpu.Context(2)
    for count in COUNTS:
        for src_off in range(4):
            for dst_off in range(2):
                x = patterns(dtype, count, seed=11 * count + 3 * src_off + dst_off)
                assert_same(widen_on_device(ctx, dtype, x, src_off, dst_off), yardstick(dtype, x), (dtype, count, src_off, dst_off))
    ctx.close()


@pytest.mark.parametrize("dtype", [F16, BF16, U16, I16, U8, I8])
def test_widen_typed_every_pattern(gpu, dtype):
    """all 65 536 patterns of a half, a bfloat16 and the 16-bit integers (all 256 of the 8-bit ones, 256 times over): this is what shows
    that the device's conversion keeps subnormal halves under the library's flags"""
    ctx = gpu.Context(2)
    x = patterns(dtype, 65536)
    exp = yardstick(dtype, x)
    if dtype in (F16, BF16):
        assert np.isnan(exp).any() and np.isinf(exp).sum() == 2 and (exp == 0).sum() == 2
        tiny = 2.0 ** -14 if dtype == F16 else float(np.finfo(np.float32).tiny)
        assert ((np.abs(exp) > 0) & (np.abs(exp) < tiny)).sum() == (2 * 1023 if dtype == F16 else 2 * 127)          # the subnormals are all there
    for src_off, dst_off in ((0, 0), (1, 1), (3, 0)):          # the body, the body behind a head, element by element
        assert_same(widen_on_device(ctx, dtype, x, src_off, dst_off), exp, (dtype, src_off, dst_off))
    ctx.close()


GRID = 2048 * 256          # lanes of the capped grid (widen_steps.hpp: kWidenMaxBlocks * kWidenThreads): one group of 4 each per round


@pytest.mark.parametrize("count,src_off,dst_off,turns", [
    (2 ** 21 + 5, 0, 0, (2, 1)),                            # no head: GRID + 1 groups -- lane 0 takes a pair, every other lane one group
    (3 + 4 * (2 * GRID + 777) + 2, 1, 1, (3, 2)),           # behind a head of 3: 777 lanes take a pair and the odd one, the others a pair
    (4 * (3 * GRID + 4321) + 1, 0, 0, (4, 3)),              # 4321 lanes two pairs, the others a pair and the odd one
])
@pytest.mark.parametrize("dtype", [U8, I16])
def test_widen_typed_grid_stride_loop(gpu, dtype, count, src_off, dst_off, turns):
    """more groups of 4 BEHIND THE HEAD than the capped grid has lanes, so the grid-stride loop goes round: two groups a turn, one grid
    apart, and the odd one at the end -- lanes with an even and lanes with an odd number of groups in every case"""
    head = (4 - src_off) % 4
    assert (head + dst_off) % 2 == 0                                               # the 4-element body
    nvec = (count - head) // 4
    assert nvec > GRID and (-(-nvec // GRID), nvec // GRID) == turns and nvec % GRID != 0
    ctx = gpu.Context(2)
    x = np.random.default_rng(dtype).integers(0, 256, size=count * np.dtype(STORAGE[dtype]).itemsize, dtype=np.uint8).view(STORAGE[dtype])
    assert_same(widen_on_device(ctx, dtype, x, src_off, dst_off), yardstick(dtype, x), (dtype, count))
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


MODES = ("host", "device 1", "device 2", "offset")


def handed(a, mode):
    """the array as the caller hands it over -> (what is pushed, on_device, a check that it is as it was, which then overwrites it).  "offset":
    a device tensor one element (for the 8-bit types: an odd number of bytes) into a larger buffer, which forces the element-wise form"""
    import torch
    if mode == "host":
        x = np.ascontiguousarray(a).copy()
        before = x.copy()

        def check():
            assert x.tobytes() == before.tobytes(), "a pushed array was written"
            x[...] = 77
        return x, None, check
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy())
    if mode == "offset":
        buf = torch.zeros(flat.numel() + 9, dtype=flat.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[1:1 + flat.numel()] = flat.cuda()
        x = buf[1:1 + flat.numel()].view(a.shape)
        assert x.is_contiguous() and x.data_ptr() == buf.data_ptr() + flat.element_size()
    else:
        x = flat.cuda().view(a.shape)
    torch.cuda.synchronize()
    before = x.clone()

    def check():
        assert torch.equal(x.view(torch.uint8), before.view(torch.uint8)), "a pushed tensor was written"
        x.fill_(77)
        torch.cuda.synchronize()
    return x, (2 if mode == "device 2" else 1), check


def sweep_all(gpu, ctx, nt):
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    recs, factors, _ = ctx.sweep_series(range(nt), scopes)
    return recs, [int(f) for f in factors]


def scalar_series(gpu, ctx, slices, mode="host", keep_dtype=True):
    """pushes the slices -- each unchanged by the push and overwritten right after it, before the sweep -- and sweeps every step in one pass"""
    for t, a in enumerate(slices):
        x, on_device, check = handed(a, mode)
        ctx.push_scalar_slice(t, x, on_device=on_device, keep_dtype=keep_dtype)
        check()
    return sweep_all(gpu, ctx, len(slices))


def vector_series(gpu, ctx, slices, mode="host", keep_dtype=True):
    for t, a in enumerate(slices):
        x, on_device, check = handed(a, mode)
        ctx.push_slice(t, x, keep_dtype=keep_dtype)
        check()
    return sweep_all(gpu, ctx, len(slices))


WOVEN_DIMS = (31, 37)
QUANTISED = {I16: ("int16", lambda a: np.round(a * 30000).astype(np.int16)), U8: ("uint8", lambda a: np.round((a + 1) * 127).astype(np.uint8)),
             F16: ("float16", lambda a: a.astype(np.float16))}


@pytest.fixture(scope="module")
def woven(gpu, oracle):
    """woven 31 x 37 x 4 quantised to int16 and to uint8, and as float16: per type the narrow slices, the widened ones, what the FP64 push of
    the widened slices gives, and the oracle's records -- computed once"""
    import torch
    from ftk_amd import synthetic
    raw = [synthetic.woven(WOVEN_DIMS, k, 4, torch, "cpu").numpy() for k in range(4)]
    out = {}
    for dtype, (_, quantise) in QUANTISED.items():
        x = [np.ascontiguousarray(quantise(a)) for a in raw]
        x64 = [a.astype(np.float64) for a in x]
        ctx = scalar_context(gpu, WOVEN_DIMS)
        fp64 = scalar_series(gpu, ctx, x64, keep_dtype=False)
        assert ctx.narrow_counts() == (0,) * 10 and ctx.f32_counts() == (0, 0)
        ctx.close()
        ref, rf, _ = oracle.track(x64, 2, 1, tag_mode=oracle.TAG_REFERENCE)
        assert len(ref) > 0 and len(fp64[0]) > 0
        out[dtype] = dict(x=x, x64=x64, fp64=fp64, oracle=(ref, [int(f) for f in rf]))
    assert not same_records(out[I16]["fp64"][0], out[U8]["fp64"][0])          # (a push that read the wrong array is seen)
    return out


def counts_of(dtype, n):
    return tuple(n if d == dtype else 0 for d in range(10))


# ---- 2. push against push, 2D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", sorted(QUANTISED))
def test_push_2d(gpu, woven, dtype, mode):
    w = woven[dtype]
    exp_recs, exp_factors = w["fp64"]
    ctx = scalar_context(gpu, WOVEN_DIMS)
    recs, factors = scalar_series(gpu, ctx, w["x"], mode)
    assert factors == exp_factors == w["oracle"][1]
    assert same_records(recs, exp_recs)                                        # bit for bit and in order
    assert_records_equal(as_fixture(recs), w["oracle"][0], coord_tol=0.0, what=f"{QUANTISED[dtype][0]} push, {mode}")
    # counters: one narrow launch per array; the float32, planar and adjust counters stay
    assert ctx.narrow_counts() == counts_of(dtype, 4) and ctx.f32_counts() == (0, 0) and ctx.planar_counts() == (0, 0) and ctx.adjust_counts() == (0, 0, 0)
    ctx.close()


# ---- 3. the same in 3D, scalar and vector --------------------------------------------------------------------------------------------------------
DIMS_3D = (9, 7, 5)


def bumps_int16(DT=3):
    """two moving Gaussian bumps of opposite sign on 9 x 7 x 5, quantised to int16 (the oracle finds 20 critical points in this one)"""
    z, y, x = np.meshgrid(np.arange(DIMS_3D[2]), np.arange(DIMS_3D[1]), np.arange(DIMS_3D[0]), indexing="ij")
    out = []
    for k in range(DT):
        S = (np.exp(-((x - 3.3 - 0.4 * k) ** 2 + (y - 3.2 - 0.2 * k) ** 2 + (z - 2.1 - 0.1 * k) ** 2) / (2 * 1.5 ** 2))
             - 0.6 * np.exp(-((x - 5.6 + 0.3 * k) ** 2 + (y - 2.7) ** 2 + (z - 2.4) ** 2) / (2 * 1.2 ** 2)))
        out.append(np.round(S * 20000).astype(np.int16))
    return out


def linear_field_int16(DT=3):
    """a linear vector field with one moving zero on 9 x 7 x 5, quantised to int16 (14 critical points)"""
    z, y, x = np.meshgrid(np.arange(DIMS_3D[2]), np.arange(DIMS_3D[1]), np.arange(DIMS_3D[0]), indexing="ij")
    out = []
    for k in range(DT):
        c = (4.3 + 0.4 * k, 3.2 + 0.3 * k, 2.4 - 0.2 * k)
        V = np.stack([(x - c[0]) + 0.3 * (y - c[1]), (y - c[1]) - 0.2 * (z - c[2]), -(z - c[2]) + 0.1 * (x - c[0])], axis=-1)
        out.append(np.ascontiguousarray(np.round(V * 1000).astype(np.int16)))
    return out


@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
def test_push_3d(gpu, oracle, vector):
    x = linear_field_int16() if vector else bumps_int16()
    x64 = [a.astype(np.float64) for a in x]
    make, series = (vector_context, vector_series) if vector else (scalar_context, scalar_series)
    ref, rf, _ = oracle.track(x64, 3, 2 if vector else 1, tag_mode=oracle.TAG_REFERENCE)
    assert len(ref) > 0
    A = make(gpu, DIMS_3D)
    exp_recs, exp_factors = series(gpu, A, x64, keep_dtype=False)
    A.close()
    for mode in MODES:
        B = make(gpu, DIMS_3D)
        recs, factors = series(gpu, B, x, mode)
        assert factors == exp_factors == [int(f) for f in rf], mode
        assert same_records(recs, exp_recs), mode
        assert_records_equal(as_fixture(recs), ref, coord_tol=0.0, what=f"int16 3D push, {mode}")
        assert B.narrow_counts() == counts_of(I16, 3) and B.f32_counts() == (0, 0)
        B.close()


# ---- 4. the resident slice ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
def test_resident_slice_is_the_widened_array(gpu, woven, vector):
    """read back through the patches the halo exchange gathers: byte for byte the array the FP64 push leaves, which is the widened array"""
    for dtype in (U8, I16, F16, BF16, I8, I32):
        rng = np.random.default_rng(dtype)
        shape = tuple(reversed(WOVEN_DIMS)) + ((2,) if vector else ())
        bits = rng.integers(0, 256, size=int(np.prod(shape)) * np.dtype(STORAGE[dtype]).itemsize, dtype=np.uint8).view(STORAGE[dtype])
        if dtype in (F16, BF16):          # finite values only: a slice holds a field
            bits = bits & np.uint16(0x3fff if dtype == F16 else 0x7eff) | (bits & np.uint16(0x8000))
        exp = yardstick(dtype, bits).reshape(shape)
        assert np.isfinite(exp).all()
        if dtype == BF16:
            import torch
            x = torch.from_numpy(bits.view(np.int16).reshape(shape).copy()).view(torch.bfloat16)
        else:
            x = bits.view(np.float16 if dtype == F16 else STORAGE[dtype]).reshape(shape).copy()
        for on_device in (False, True):
            if on_device:
                import torch
                x = (x if hasattr(x, "data_ptr") else torch.from_numpy(x)).cuda()
            M, N = Mesh(gpu, WOVEN_DIMS, vector), Mesh(gpu, WOVEN_DIMS, vector)
            if vector:
                M.ctx.push_slice(0, x, keep_dtype=True); N.ctx.push_slice(0, exp)
            else:
                M.ctx.push_scalar_slice(0, x, keep_dtype=True); N.ctx.push_scalar_slice(0, exp)
            got, ref = M.read(0), N.read(0)
            assert got.tobytes() == ref.tobytes() == exp.tobytes(), (dtype, vector, on_device)
            assert M.ctx.narrow_counts() == counts_of(dtype, 1)
            M.close(); N.close()


# ---- 5. the chain behind the widening ------------------------------------------------------------------------------------------------------------
def chained(gpu, slices, setting, keep_dtype, mode="host"):
    """the 31 x 37 series under one setting of the chain -> (records, factors, the context's counters)"""
    ctx = scalar_context(gpu, WOVEN_DIMS)
    if setting == "smooth":
        ctx.set_spatial_smoothing(1.0, 3)
    elif setting == "clamp":
        ctx.set_clamp(float(np.percentile(slices[0].astype(np.float64), 20)), float(np.percentile(slices[0].astype(np.float64), 80)))
    elif setting == "perturb":
        ctx.set_perturbation(0.01 * float(np.abs(slices[0].astype(np.float64)).max()), 12345)
    elif setting == "smooth+perturb":          # (the pooled array, the convolution and the adjust kernel in one chain)
        ctx.set_spatial_smoothing(1.0, 3)
        ctx.set_perturbation(0.01 * float(np.abs(slices[0].astype(np.float64)).max()), 12345)
    if setting == "temporal":
        ctx.set_temporal_smoothing(1.0, 3, 0)
        emitted = []
        for a in slices:
            x, on_device, check = handed(a, mode)
            t = ctx.temporal_push(x, on_device=on_device, keep_dtype=keep_dtype)
            check()
            if t >= 0:
                emitted.append(t)
        while True:
            t = ctx.temporal_flush()
            if t < 0:
                break
            emitted.append(t)
        assert emitted == list(range(len(slices)))
        out = sweep_all(gpu, ctx, len(emitted))
    else:
        out = scalar_series(gpu, ctx, slices, mode, keep_dtype=keep_dtype)
    counters = dict(narrow=ctx.narrow_counts(), f32=ctx.f32_counts(), adjust=ctx.adjust_counts(), planar=ctx.planar_counts())
    ctx.close()
    return out[0], out[1], counters


@pytest.mark.parametrize("setting", ["smooth", "clamp", "perturb", "smooth+perturb", "temporal"])
def test_chain_behind_the_widening(gpu, woven, setting):
    """spatial smoothing ksize 3, clamp, perturbation (seed 12345), smoothing with perturbation, and temporal smoothing K = 3 through ftkx_temporal_push_typed:
    byte-identical to the FP64 push of the widened array under the same settings -- and the settings did something"""
    for dtype in (I16, U8):
        w = woven[dtype]
        exp_recs, exp_factors, exp_cnt = chained(gpu, w["x64"], setting, False)
        assert len(exp_recs) > 0 and not same_records(exp_recs, w["fp64"][0]), setting
        assert exp_cnt["narrow"] == (0,) * 10
        for mode in (("host", "device 1", "offset") if dtype == I16 else ("host", "device 2")):
            recs, factors, cnt = chained(gpu, w["x"], setting, True, mode)
            assert factors == exp_factors and same_records(recs, exp_recs), (setting, dtype, mode)
            assert cnt["narrow"] == counts_of(dtype, 4) and cnt["f32"] == (0, 0) and cnt["planar"] == (0, 0), (setting, dtype, mode)
            # as for an FP64 source copied into the slice: adjusted in place, once per array, where perturbation or clamp is set
            assert cnt["adjust"] == ((0, 4, 0) if ("clamp" in setting or "perturb" in setting) else (0, 0, 0)), (setting, dtype, mode)


# ---- 6. order ------------------------------------------------------------------------------------------------------------------------------------
def test_narrow_float32_and_float64_pushes_alternate(gpu, woven):
    """one context, one staging block: int16, float32 and FP64 pushes of the same values in turn, host and device sources among them"""
    import torch
    w = woven[I16]
    ctx = scalar_context(gpu, WOVEN_DIMS)
    for t in range(4):
        ctx.push_scalar_slice(2 * t, w["x"][t] if t % 2 == 0 else torch.from_numpy(w["x"][t]).cuda(), keep_dtype=True)
        ctx.drop_slice(2 * t)
        ctx.push_scalar_slice(t, [w["x"][t], w["x64"][t].astype(np.float32), w["x64"][t], torch.from_numpy(w["x"][t]).cuda()][t], keep_dtype=True)
    recs, factors = sweep_all(gpu, ctx, 4)
    assert factors == w["fp64"][1] and same_records(recs, w["fp64"][0])          # (|x| <= 30000: exact in float32 too)
    assert ctx.narrow_counts() == counts_of(I16, 6) and ctx.f32_counts() == (1, 0)
    ctx.close()


# ---- 7. the tracker and the Python layer ---------------------------------------------------------------------------------------------------------
def tracked(gpu, slices, keep_dtype, device=False, device_ids=None):
    import torch
    tr = gpu.CriticalPointTracker2DRegular(device_ids=device_ids)
    try:
        tr.set_scalar_field_source(gpu.SOURCE_GIVEN); tr.set_vector_field_source(gpu.SOURCE_DERIVED)
        tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
        tr.set_domain([2, 2], [d - 3 for d in WOVEN_DIMS]); tr.set_array_domain([0, 0], list(WOVEN_DIMS))
        tr.initialize()
        for k, a in enumerate(slices):
            if device:
                a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                torch.cuda.synchronize()
            tr.push_scalar_field_snapshot(a, keep_dtype=keep_dtype)
            if device:
                a.fill_(77)                    # (a narrow snapshot is read before the push returns)
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


def test_tracker_takes_uint8_frames(gpu, woven):
    w = woven[U8]
    exp = tracked(gpu, w["x64"], False)
    assert len(exp[0]) > 0 and len(exp[3]) > 0
    for device in (False, True):
        got = tracked(gpu, w["x"], True, device=device)
        assert same_records(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
        assert got[3] == exp[3] and got[4] == exp[4]
    with pytest.raises(gpu.FtkxError) as e:
        tracked(gpu, w["x"], True, device_ids=[0, 0])
    assert e.value.code == gpu._lib.E_UNSUPPORTED


def test_element_types_of_the_python_layer(gpu, woven):
    import torch
    w = woven[I16]
    shape = tuple(reversed(WOVEN_DIMS))
    ctx = scalar_context(gpu, WOVEN_DIMS)
    # keep_dtype=True: what the library does not take raises TypeError before any call into it
    for bad in (np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=bool), np.zeros(shape, dtype=np.complex64),
                np.zeros(shape, dtype=np.dtype(">i2")), torch.zeros(shape, dtype=torch.int64), torch.zeros(shape, dtype=torch.bool)):
        with pytest.raises(TypeError):
            ctx.push_scalar_slice(0, bad, keep_dtype=True)
        with pytest.raises(TypeError):
            ctx.push_slice(0, bad, keep_dtype=True)
    with pytest.raises(TypeError):
        ctx.push_slice(0, np.zeros(shape + (2,), dtype=np.int16), np.zeros(shape + (2, 2), dtype=np.int32), keep_dtype=True)          # one push, two element types
    assert ctx.narrow_counts() == (0,) * 10
    # without keep_dtype: a float16 tensor still raises, an int32 numpy array still takes the host-widened FP64 path
    with pytest.raises(TypeError):
        ctx.push_scalar_slice(0, torch.zeros(shape, dtype=torch.float16))
    ctx.push_scalar_slice(0, w["x"][0].astype(np.int32))
    assert ctx.narrow_counts() == (0,) * 10 and ctx.f32_counts() == (0, 0)
    # with it: float32 and float64 go where they go today
    ctx.push_scalar_slice(1, w["x64"][1].astype(np.float32), keep_dtype=True)
    ctx.push_scalar_slice(2, w["x64"][2], keep_dtype=True)
    assert ctx.narrow_counts() == (0,) * 10 and ctx.f32_counts() == (1, 0)
    # ... and every narrow type of numpy and of torch is taken as it is
    for k, a in enumerate((np.zeros(shape, dtype=np.float16), np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.int8), np.zeros(shape, dtype=np.uint16),
                           np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.int32))):
        ctx.push_scalar_slice(3, a, keep_dtype=True)
    assert ctx.narrow_counts() == (0, 0, 1, 0, 1, 1, 1, 1, 1, 1)
    for a in (torch.zeros(shape, dtype=torch.float16), torch.zeros(shape, dtype=torch.bfloat16), torch.zeros(shape, dtype=torch.uint8), torch.zeros(shape, dtype=torch.int8),
              torch.zeros(shape, dtype=torch.int16), torch.zeros(shape, dtype=torch.int32)):
        ctx.push_scalar_slice(3, a, keep_dtype=True)
        ctx.push_scalar_slice(3, a.cuda(), keep_dtype=True)
    assert ctx.narrow_counts() == (0, 0, 3, 2, 3, 3, 1, 3, 1, 3)
    ctx.close()


def test_views_that_are_not_contiguous(gpu, woven):
    """a channel of an interleaved image (img[..., 1]) and every other column of a wider frame, uint8 and int16, host and device, through
    Context and through the tracker: the push reads a contiguous copy, which lives until the library has read it -- the frames' other
    channels hold other values, and memory is churned between the copy and the check, so a read of anything else is seen"""
    import torch
    for dtype in (U8, I16):
        w = woven[dtype]
        views = []
        for a in w["x"]:
            img = np.stack([a[::-1], a, a.T.reshape(a.shape)], axis=-1).copy()
            wide = np.repeat(a, 2, axis=1); wide[:, 1::2] += 3
            views.append((img[..., 1], wide[:, ::2]))
            assert not img[..., 1].flags.c_contiguous and not wide[:, ::2].flags.c_contiguous
            assert np.array_equal(img[..., 1], a) and np.array_equal(wide[:, ::2], a)
        for device in (False, True):
            for which in (0, 1):
                ctx = scalar_context(gpu, WOVEN_DIMS)
                for t in range(4):
                    v = views[t][which]
                    if device:
                        base = torch.from_numpy(np.ascontiguousarray(v.base if v.base is not None else v)).cuda()
                        v = base[..., 1] if which == 0 else base[:, ::2]
                        assert not v.is_contiguous()
                    ctx.push_scalar_slice(t, v, keep_dtype=True)
                    junk = [np.full(v.shape, 55, dtype=w["x"][0].dtype) for _ in range(4)]          # (what a freed copy would be overwritten by)
                    if device:
                        junk += [torch.full(tuple(v.shape), 55, dtype=v.dtype, device="cuda") for _ in range(4)]
                recs, factors = sweep_all(gpu, ctx, 4)
                assert factors == w["fp64"][1] and same_records(recs, w["fp64"][0]), (dtype, device, which)
                assert ctx.narrow_counts() == counts_of(dtype, 4)
                ctx.close()
    # ... and the tracker, whose push goes through one more function between the copy and the call
    w = woven[U8]
    exp = tracked(gpu, w["x64"], False)
    frames = [np.stack([a[::-1], a], axis=-1).copy()[..., 1] for a in w["x"]]
    assert not frames[0].flags.c_contiguous
    got = tracked(gpu, frames, True)
    assert same_records(got[0], exp[0]) and got[3] == exp[3] and got[4] == exp[4]
    got = tracked(gpu, [torch.from_numpy(np.stack([a[::-1], a], axis=-1).copy()).cuda()[..., 1] for a in w["x"]], True)
    assert same_records(got[0], exp[0]) and got[3] == exp[3] and got[4] == exp[4]


# ---- 8. contract errors: the codes of the FP64 entries --------------------------------------------------------------------------------------------
def test_contract_errors(gpu):
    import torch
    L = gpu._lib.load()
    E, U = gpu._lib.E_INVALID, gpu._lib.E_UNSUPPORTED
    a16 = np.zeros((12, 16), dtype=np.int16); a64 = np.zeros((12, 16)); v16 = np.zeros((12, 16, 2), dtype=np.int16); v64 = np.zeros((12, 16, 2))
    t = C.c_int(0)
    assert [L.ftkx_dtype_size(d) for d in range(-1, 12)] == [0, 8, 4, 2, 2, 1, 1, 2, 2, 4, 4, 0, 0]
    ctx = gpu.Context(2)
    h = ctx._h
    assert L.ftkx_push_scalar_slice_typed(h, 0, a16.ctypes.data, I16, 0) == L.ftkx_push_scalar_slice(h, 0, a64.ctypes.data, 0) == E          # before ftkx_set_mesh
    ctx.set_mesh(([1, 1], [14, 10]), ([1, 1], [14, 10]), ([0, 0], [16, 12]))
    ctx.set_options(jacobian_symmetric=0, derive_jacobian=1)
    assert L.ftkx_push_scalar_slice_typed(None, 0, a16.ctypes.data, I16, 0) == E
    for bad in (-1, 10, 11, 64):                                                                            # unknown dtype (64-bit integers have no code)
        assert L.ftkx_push_scalar_slice_typed(h, 0, a16.ctypes.data, bad, 0) == E
        assert L.ftkx_push_slice_typed(h, 0, v16.ctypes.data, None, None, bad, 0) == E
        assert L.ftkx_temporal_push_typed(h, a16.ctypes.data, bad, 0, 0, C.byref(t)) == E
    assert L.ftkx_push_scalar_slice_typed(h, 0, a16.ctypes.data + 1, I16, 0) == E                           # not a multiple of the element's size
    assert L.ftkx_push_scalar_slice_typed(h, 0, a16.ctypes.data + 2, I32, 0) == E
    assert L.ftkx_push_slice_typed(h, 0, v16.ctypes.data, v16.ctypes.data + 1, None, I16, 0) == E
    assert L.ftkx_push_scalar_slice_typed(h, 0, None, I16, 0) == L.ftkx_push_scalar_slice(h, 0, None, 0) == E
    assert L.ftkx_push_slice_typed(h, 0, None, None, a16.ctypes.data, I16, 0) == L.ftkx_push_slice(h, 0, None, None, a64.ctypes.data, 0) == E
    assert L.ftkx_push_scalar_slice_typed(h, 0, a16.ctypes.data, I16, 3) == L.ftkx_push_scalar_slice(h, 0, a64.ctypes.data, 3) == E
    assert L.ftkx_push_scalar_slice_typed(h, -1, a16.ctypes.data, I16, 0) == L.ftkx_push_scalar_slice(h, -1, a64.ctypes.data, 0) == E
    assert L.ftkx_temporal_push_typed(h, a16.ctypes.data, I16, 0, 0, C.byref(t)) == L.ftkx_temporal_push(h, a64.ctypes.data, 0, 0, C.byref(t)) == E      # no filter set
    ctx.set_spatial_smoothing(1.0, 3)
    assert L.ftkx_push_slice_typed(h, 0, v16.ctypes.data, None, None, I16, 0) == L.ftkx_push_slice(h, 0, v64.ctypes.data, None, None, 0) == U
    ctx.set_temporal_smoothing(1.0, 3, 0)
    assert L.ftkx_temporal_push_typed(h, v16.ctypes.data, I16, 1, 0, C.byref(t)) == L.ftkx_temporal_push(h, v64.ctypes.data, 1, 0, C.byref(t)) == U
    assert L.ftkx_temporal_push_typed(h, a16.ctypes.data, I16, 0, 0, None) == E
    ctx.set_temporal_smoothing(0.0, 0, 0)
    ctx.set_spatial_smoothing(0.0, 0)
    ctx.set_clamp(-1.0, 1.0)                                                                                # adjust refuses J or S beside V
    assert L.ftkx_push_slice_typed(h, 0, v16.ctypes.data, None, a16.ctypes.data, I16, 0) == L.ftkx_push_slice(h, 0, v64.ctypes.data, None, a64.ctypes.data, 0) == U
    ctx.set_clamp()
    assert ctx.narrow_counts() == (0,) * 10                                                                 # nothing of all that was launched
    # the stand-alone entries
    s = torch.zeros(64, dtype=torch.int16, device="cuda"); d = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert L.ftkx_widen_typed(h, None, I16, 8, d.data_ptr()) == E and L.ftkx_widen_typed(h, s.data_ptr(), I16, 8, None) == E
    assert L.ftkx_widen_typed(h, s.data_ptr(), I16, 0, d.data_ptr()) == E                                   # count 0
    assert L.ftkx_widen_typed(h, s.data_ptr() + 1, I16, 8, d.data_ptr()) == E and L.ftkx_widen_typed(h, s.data_ptr(), I16, 8, d.data_ptr() + 4) == E      # misaligned
    assert L.ftkx_widen_typed(h, s.data_ptr() + 2, U32, 8, d.data_ptr()) == E
    assert L.ftkx_widen_typed(h, s.data_ptr(), 10, 8, d.data_ptr()) == E and L.ftkx_widen_typed(h, s.data_ptr(), -1, 8, d.data_ptr()) == E                 # unknown dtype
    assert L.ftkx_widen_typed(h, d.data_ptr() + 16, I16, 8, d.data_ptr()) == E                              # overlapping
    ms = (C.c_double * 2)()
    assert L.ftkx_debug_narrow_relaunch(h, s.data_ptr(), I16, 8, d.data_ptr(), 0, ms) == E
    assert L.ftkx_debug_narrow_relaunch(h, s.data_ptr(), I16, 8, d.data_ptr(), 2, ms) == 0 and ms[0] >= 0
    assert L.ftkx_debug_narrow_relaunch(h, s.data_ptr(), F32, 8, d.data_ptr(), 2, ms) == 0                  # float32: the widen kernel's relaunch
    assert L.ftkx_debug_narrow_relaunch(h, s.data_ptr(), F64, 8, d.data_ptr(), 2, ms) == E
    buf = C.create_string_buffer(512)
    L.ftkx_last_error(h, buf, 512)
    assert b"FTKX_DTYPE_F16 .. FTKX_DTYPE_I32" in buf.value, buf.value
    assert L.ftkx_debug_narrow_counts(None, None) == E and L.ftkx_debug_narrow_counts(h, None) == E
    ctx.close()
