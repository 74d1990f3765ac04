"""Vector snapshots given as one array per component (ftk_amd/csrc/concat_kernels.hip, concat_steps.hpp): the planes go to the device as
they are, float32 or FP64, and one kernel writes the interleaved FP64 V -- what the reference's stream does on the host with
ndarray<T>::concat when a file keeps u, v, w in separate variables.  Interleaving moves values and widening is exact, so there is no
tolerance anywhere in this file: the kernel is held to numpy's stack + astype as 64-bit integers (tests/test_concat_golden.py holds that
expression to the real reference), and a planar push gives, byte for byte, what push_slice of the host-interleaved array gives -- plain,
with perturbation and clamp, with temporal smoothing, and through the tracker, where it is the reference's own records."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import assert_records_equal, load_golden
from test_gpu_f32 import SPECIAL as SPECIAL32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(ROOT, "ftk_amd", "csrc", "concat_steps.hpp")).read())
    assert m, name
    return int(m.group(1))


THREADS, MAX_BLOCKS = _constant("kConcatThreads"), _constant("kConcatMaxBlocks")


def group(dtype):
    return 16 // np.dtype(dtype).itemsize          # vertices per 16-byte load of a plane (concat_steps.hpp: concat_group)


def one_round(dtype):
    return MAX_BLOCKS * THREADS * group(dtype)     # vertices one round of the capped grid takes


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def interleave(planes):
    """THE oracle (held to the reference's concat by tests/test_concat_golden.py): components fastest, then widened"""
    with np.errstate(invalid="ignore"):
        return np.stack(list(planes), axis=-1).reshape(-1).astype(np.float64)


def wide(a):
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)


# ---- 1. the kernel against numpy ---------------------------------------------------------------------------------------------------------------
SPECIAL64 = np.array([0x0000000000000000, 0x8000000000000000,              # +-0
                      0x7ff0000000000000, 0xfff0000000000000,              # +-inf
                      0x7fefffffffffffff, 0xffefffffffffffff,              # the largest normal
                      0x0010000000000000, 0x8010000000000000,              # the smallest normal
                      0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff, 0x8000000000000123,      # subnormals
                      0x7ff8000000000000, 0xfff8000000000000,              # quiet NaNs of both signs
                      0x7ff8000000abcdef, 0xfffc0000deadbeef,              # ... with payloads
                      0x7ff0000000000001, 0xfff4000000000123], dtype=np.uint64)      # signalling NaNs: moved, never computed with


def plane_values(dtype, nc, count, seed):
    """nc planes of `count` values: random bit patterns (every exponent; NaNs and infinities among them), the special values at the front
    and (where there is room) at the back of every plane, rolled from plane to plane, so that they meet the head, the body and the tail"""
    rng = np.random.default_rng(seed)
    f32 = np.dtype(dtype) == np.float32
    bits = rng.integers(0, 2 ** 32, size=(nc, count), dtype=np.uint64).astype(np.uint32) if f32 else rng.integers(0, 2 ** 64, size=(nc, count), dtype=np.uint64)
    for k in range(nc):
        sp = np.roll(SPECIAL32 if f32 else SPECIAL64, seed + 5 * k)
        m = min(count, len(sp))
        bits[k, :m] = sp[:m]
        if count >= 2 * len(sp):
            bits[k, -len(sp):] = sp[::-1]
    return bits.view(dtype)


def kernel_counts(dtype):
    R = one_round(dtype)
    return [1, 2, 3, 4, 5, 7, 255, 256, 257, R - 1, R, R + 1]


KERNEL_CASES = [(np.dtype(t).name, nc, i) for t in (np.float32, np.float64) for nc in (2, 3) for i in range(12)]


@pytest.mark.parametrize("dtype,nc,which", KERNEL_CASES, ids=["%s-nc%d-count%d" % c for c in KERNEL_CASES])
def test_concat_against_numpy(gpu, dtype, nc, which):
    """ftkx_concat / ftkx_concat_f32 == numpy's interleave + astype as 64-bit integers (a NaN that was widened: is NaN, same sign; FP64: the
    full payload), for every common plane offset 0 .. G - 1 elements crossed with destinations 0 and 1 doubles behind a 16-byte border, and
    for one plane at another offset than the rest; the canaries on both sides of the destination stay, the planes are unchanged, and
    planar_counts() names the path the plan's rule gives"""
    import torch
    dtype = np.dtype(dtype)
    f32 = dtype == np.float32
    G, count = group(dtype), kernel_counts(dtype)[which]
    tdtype, idtype = (torch.float32, torch.int32) if f32 else (torch.float64, torch.int64)
    ctx = gpu.Context(2)
    pad = 4                                                   # doubles in front of the destination: the 16-byte border is kept
    x = plane_values(dtype, nc, count, 7 * which + nc)
    exp = interleave(x)
    nan = np.isnan(exp)
    host = [torch.from_numpy(x[k].copy()).view(idtype) for k in range(nc)]
    differing = [[(o if k else (o + 1) % G) for k in range(nc)] for o in (1,)]           # plane 0 one element off the others
    cases = [([o] * nc, d) for o in range(G) for d in (0, 1)] + [(off, 0) for off in differing]
    dst = torch.empty(count * nc + 2 * pad + 2, dtype=torch.float64, device="cuda")
    src = [torch.zeros(count + 8, dtype=tdtype, device="cuda") for _ in range(nc)]
    assert dst.data_ptr() % 16 == 0 and all(s.data_ptr() % 16 == 0 for s in src)
    seen_vec = seen_scalar = 0
    for off, dst_off in cases:
        for k in range(nc):
            src[k].view(idtype)[off[k]:off[k] + count] = host[k].cuda()
        dst.fill_(777.0)
        torch.cuda.synchronize()
        before = ctx.planar_counts()
        ctx.concat([src[k].data_ptr() + dtype.itemsize * off[k] for k in range(nc)], count, dst.data_ptr() + 8 * (pad + dst_off), f32=f32)
        after = ctx.planar_counts()
        agree = len(set(off)) == 1
        vec = agree and (dst_off + ((G - off[0]) % G) * nc) % 2 == 0          # the destination on 16 bytes behind the planes' common head
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if vec else (0, 1)), (count, off, dst_off)
        seen_vec += vec; seen_scalar += not vec
        got = dst.cpu().numpy()
        lo = pad + dst_off
        assert np.all(got[:lo] == 777.0) and np.all(got[lo + count * nc:] == 777.0), (count, off, dst_off, "a canary was written")
        for k in range(nc):
            assert torch.equal(src[k].view(idtype)[off[k]:off[k] + count].cpu(), host[k]), "a plane was written"
        out = got[lo:lo + count * nc]
        if f32:
            assert np.array_equal(np.isnan(out), nan) and np.array_equal(np.signbit(out[nan]), np.signbit(exp[nan])), (count, off, dst_off)
            assert np.array_equal(out.view(np.uint64)[~nan], exp.view(np.uint64)[~nan]), (count, off, dst_off)
        else:
            assert np.array_equal(out.view(np.uint64), exp.view(np.uint64)), (count, off, dst_off)
    assert seen_vec == G and seen_scalar == G + 1 and (count < 64 or nan.any())
    ctx.close()


# ---- the push path -----------------------------------------------------------------------------------------------------------------------------
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


def sweep_steps(gpu, ctx, ts):
    scopes = [gpu.SCOPE_BOTH if i + 1 < len(ts) else gpu.SCOPE_ORDINAL for i in range(len(ts))]
    recs, factors, _ = ctx.sweep_series(list(ts), scopes)
    return recs, [int(f) for f in factors]


def components(V, dtype, form, on_device):
    """the planes of the interleaved array V (..., nc) as the caller holds them: `separate` arrays of their own, or the leading slices of
    one `stacked` (nc, ...) array; host arrays or device tensors"""
    import torch
    nc = V.shape[-1]
    stacked = np.ascontiguousarray(np.moveaxis(V, -1, 0), dtype=dtype)
    if form == "stacked":
        return torch.from_numpy(stacked.copy()).cuda() if on_device else stacked.copy()
    planes = [stacked[k].copy() for k in range(nc)]
    return [torch.from_numpy(p).cuda() for p in planes] if on_device else planes


def handed(a, dtype, on_device):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).cuda() if on_device else a.copy()


def overwrite(x):
    """the pushed arrays are overwritten at once: the context owns what it needs"""
    import torch
    for a in (x if isinstance(x, list) else [x]):
        if a is None:
            continue
        if hasattr(a, "data_ptr"):
            a.fill_(777.0)
        else:
            a[...] = 777.0
    torch.cuda.synchronize()


def field3d(dims=(13, 11, 9), DT=3):
    """a 3D vector field with 19 critical points in three timesteps (the oracle's count), rounded to float32"""
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    out = []
    for t in range(DT):
        u = np.sin(0.5 * x + 0.3 * t) + 0.3 * np.cos(0.4 * z)
        v = np.cos(0.45 * y - 0.2 * t) + 0.3 * np.sin(0.5 * x)
        w = np.sin(0.6 * z + 0.1 * t) - 0.3 * np.cos(0.35 * y)
        out.append(np.stack([u, v, w], axis=-1).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def meshes(gpu, oracle):
    """per mesh: the float32-representable series, J and S beside it, what push_slice of the interleaved FP64 arrays gives, and the oracle's
    records -- computed once"""
    import torch
    from ftk_amd import synthetic
    out = {}
    for name, V32 in (("gyre2d", [synthetic.double_gyre((33, 29), k, torch, "cpu").numpy().astype(np.float32) for k in range(3)]), ("field3d", field3d())):
        nd = V32[0].shape[-1]
        dims = tuple(reversed(V32[0].shape[:-1]))
        V = [wide(a) for a in V32]
        J = [wide((oracle.jacobian2D(v, 0) if nd == 2 else oracle.jacobian3D(v))) for v in V]
        S = [wide(np.sqrt((v * v).sum(axis=-1))) for v in V]
        ref, rf, _ = oracle.track(V, nd, nd, tag_mode=oracle.TAG_REFERENCE)
        assert len(ref) > 0
        m = dict(dims=dims, nd=nd, V=V, J=J, S=S, oracle=(ref, [int(f) for f in rf]))
        for key, (jj, ss) in (("plain", (None, None)), ("given", (J, S))):
            ctx = vector_context(gpu, dims)
            for t in range(len(V)):
                ctx.push_slice(t, V[t], None if jj is None else jj[t], None if ss is None else ss[t])
            m[key] = sweep_steps(gpu, ctx, range(len(V)))
            assert ctx.planar_counts() == (0, 0)                      # nothing planar was asked for: the kernel never ran
            ctx.close()
        assert m["plain"][1] == m["oracle"][1]
        assert_records_equal(as_fixture(m["plain"][0]), ref, coord_tol=0.0, what=name + ", interleaved push")
        out[name] = m
    return out


# ---- 2. push against push ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("mesh", ["gyre2d", "field3d"])
def test_planar_push_is_the_interleaved_push(gpu, meshes, mesh, dtype, on_device):
    import torch
    m = meshes[mesh]
    dtype = np.dtype(dtype)
    V, nt = m["V"], len(m["V"])
    for form in ("separate", "stacked"):
        for given in (False, True):
            ctx = vector_context(gpu, m["dims"])
            for t in range(nt):
                planes = components(V[t], dtype, form, on_device)
                kept = [p.clone() for p in planes] if isinstance(planes, list) and on_device else None
                j, s = (handed(m["J"][t], dtype, on_device), handed(m["S"][t], dtype, on_device)) if given else (None, None)
                ctx.push_slice_planar(t, planes, j, s, on_device=on_device if on_device else None)
                if kept is not None:
                    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(planes, kept)), "a pushed plane was written"
                overwrite(planes)
                if dtype == np.float32 or on_device != 1:           # (FP64 J and S of this device are borrowed, as in push_slice)
                    overwrite([j, s])
            recs, factors = sweep_steps(gpu, ctx, range(nt))
            vec, scalar = ctx.planar_counts()
            assert vec + scalar == nt
            if dtype == np.float32 and on_device != 1:              # staged floats: every plane on 16 bytes
                assert (vec, scalar) == (nt, 0)
            ctx.close()
            exp_recs, exp_factors = m["given" if given else "plain"]
            assert len(recs) > 0 and factors == exp_factors, (form, given)
            assert same_records(recs, exp_recs), (form, given)
            if not given:
                assert_records_equal(as_fixture(recs), m["oracle"][0], coord_tol=0.0, what=f"planar push {mesh} {dtype} on_device {on_device} {form}")
    # the planes in another order give other records: a wrong interleave would be seen
    ctx = vector_context(gpu, m["dims"])
    for t in range(nt):
        planes = components(V[t], dtype, "separate", on_device)
        ctx.push_slice_planar(t, planes[::-1], on_device=on_device if on_device else None)
    recs, _ = sweep_steps(gpu, ctx, range(nt))
    ctx.close()
    assert not same_records(recs, m["plain"][0])


# ---- 3. the order with the other steps of the stream ----------------------------------------------------------------------------------------------
SIGMA, SEED, CLAMP = 0.01, 20240607, (-0.25, 0.2)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_perturbation_and_clamp_behind_the_concat(gpu, meshes, dtype, on_device):
    """concat -> perturb -> clamp: the planar push gives what the interleaved push gives under the same settings (the noise's index is the
    flat index of the interleaved array), through ONE in-place launch of the adjust kernel per push"""
    m = meshes["gyre2d"]
    dtype = np.dtype(dtype)
    V, nt = m["V"], len(m["V"])
    A = vector_context(gpu, m["dims"])
    A.set_perturbation(SIGMA, SEED); A.set_clamp(*CLAMP)
    for t in range(nt):
        A.push_slice(t, handed(V[t], dtype, on_device))
    exp = sweep_steps(gpu, A, range(nt))
    A.close()
    assert len(exp[0]) > 0 and not same_records(exp[0], m["plain"][0])
    B = vector_context(gpu, m["dims"])
    B.set_perturbation(SIGMA, SEED); B.set_clamp(*CLAMP)
    for t in range(nt):
        planes = components(V[t], dtype, "separate" if t % 2 else "stacked", on_device)
        before = B.adjust_counts()
        B.push_slice_planar(t, planes)
        after = B.adjust_counts()
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, 1, 0)
        overwrite(planes)
    got = sweep_steps(gpu, B, range(nt))
    assert sum(B.planar_counts()) == nt
    B.close()
    assert got[1] == exp[1] and same_records(got[0], exp[0])


@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_temporal_filter_behind_the_concat(gpu, dtype, on_device):
    """concat -> temporal filter (ksize 5): temporal_push_planar gives the emissions, and the records, of temporal_push of the interleaved array"""
    import torch
    from ftk_amd import synthetic
    dims, DT = (33, 29), 7
    dtype = np.dtype(dtype)
    V = [wide(synthetic.double_gyre(dims, k, torch, "cpu").numpy()) for k in range(DT)]

    def run(push):
        ctx = vector_context(gpu, dims)
        ctx.set_temporal_smoothing(1.0, 5, 0)
        ts = [t for t in (push(ctx, a) for a in V) if t >= 0]
        while True:
            t = ctx.temporal_flush()
            if t < 0:
                break
            ts.append(t)
        out = (ts,) + sweep_steps(gpu, ctx, ts)
        counts = ctx.planar_counts()
        ctx.close()
        return out, counts

    def planar(ctx, a):
        planes = components(a, dtype, "separate", on_device)
        t = ctx.temporal_push_planar(planes, on_device=on_device if on_device else None)
        overwrite(planes)
        return t

    exp, none = run(lambda ctx, a: ctx.temporal_push(handed(a, dtype, on_device), is_vector=True, on_device=on_device if on_device else None))
    got, counts = run(planar)
    assert none == (0, 0) and sum(counts) == DT
    assert exp[0] == list(range(DT)) and got[0] == exp[0] and got[2] == exp[2]
    assert len(exp[1]) > 0 and same_records(got[1], exp[1])


# ---- 4. the tracker on the reference's fixtures ----------------------------------------------------------------------------------------------
def vector_tracker(gpu, g, **kw):
    nd = g["nd"]
    T = gpu.CriticalPointTracker2DRegular if nd == 2 else gpu.CriticalPointTracker3DRegular
    tr = T(**kw)
    shp = g["steps"][0].shape[:nd]
    D = [shp[nd - 1 - d] for d in range(nd)]
    tr.set_scalar_field_source(gpu.SOURCE_NONE); tr.set_vector_field_source(gpu.SOURCE_GIVEN)      # json_interface.hh:646-656
    tr.set_jacobian_field_source(gpu.SOURCE_DERIVED); tr.set_jacobian_symmetric(False)
    tr.set_domain([1] * nd, [d - 2 for d in D]); tr.set_array_domain([0] * nd, D)
    tr.set_enable_robust_detection(g["robust"])
    if g["type_filter"] is not None:
        tr.set_type_filter(g["type_filter"])
    tr.set_enable_computing_degrees(g["degrees"])
    tr.set_tag_mode(gpu.TAG_REFERENCE)
    return tr


def planes_of(V, device=False, dtype=np.float64):
    """the interleaved snapshot de-interleaved with numpy, as a reader of per-variable files would hold it"""
    import torch
    planes = [np.ascontiguousarray(V[..., k], dtype=dtype) for k in range(V.shape[-1])]
    return [torch.from_numpy(p).cuda() for p in planes] if device else planes


def points_as_fixture(points):
    recs, o, ts = points
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = o; out["timestep"] = ts
    return out


def track_components(gpu, g, device=False, dtype=np.float64, interleaved=False, temporal=None):
    tr = vector_tracker(gpu, g)
    if temporal:
        tr.set_temporal_smoothing(*temporal)
    tr.initialize()
    factors, n = [], 0

    def arrived():
        nonlocal n
        if n:
            tr.advance_timestep()
            factors.append(int(tr.get_vector_field_scaling_factor()))
        n += 1

    for V in g["steps"]:
        if interleaved:
            tr.push_vector_field_snapshot(np.ascontiguousarray(V, dtype=dtype))
        else:
            planes = planes_of(V, device, dtype)
            tr.push_vector_field_components(planes)
            overwrite(planes)
        if tr.snapshots_from_last_push():
            arrived()
    while temporal and tr.flush_temporal_smoothing():
        arrived()
    tr.update_timestep()
    factors.append(int(tr.get_vector_field_scaling_factor()))
    points = tr.get_critical_points()
    tr.close()
    return points_as_fixture(points), factors


TRACKER_FIXTURES = ["double_gyre_64x32x50", "random_2d_vector_23x20x5", "adversarial_3d_vector_8x8x8x3", "huge_nan_2d_vector_16x14x4"]


@pytest.mark.parametrize("name", TRACKER_FIXTURES)
def test_tracker_components_match_reference_fixture(gpu, name):
    g = load_golden(name)
    assert g["nv"] == g["nd"] and g["bounds"] is None and g["rectilinear"] is None and g["explicit"] is None and not g["t0"]
    for device in (False, True):
        recs, factors = track_components(gpu, g, device=device)
        assert factors == [int(f) for f in g["factors"]], "per-step quantisation factor differs from the reference"
        assert_records_equal(recs, g["records"], coord_tol=0.0, what=f"{name}, components, device {device} (bit-exact)")


def test_tracker_float32_components_and_temporal_smoothing(gpu):
    """float32 planes give what the float32 interleaved snapshot gives; with temporal smoothing on, planes give what the interleaved array gives"""
    g = load_golden("random_2d_vector_23x20x5")
    exp = track_components(gpu, g, dtype=np.float32, interleaved=True)
    got = track_components(gpu, g, dtype=np.float32)
    assert len(exp[0]) > 0 and got[1] == exp[1] and same_records(got[0], exp[0])
    exp = track_components(gpu, g, interleaved=True, temporal=(1.0, 3))
    for device in (False, True):
        got = track_components(gpu, g, device=device, temporal=(1.0, 3))
        assert len(exp[0]) > 0 and got[1] == exp[1] and same_records(got[0], exp[0])


def test_two_slab_ranks_push_components(gpu):
    """two trackers, one per rank and thread, over the in-process hub on one device, each pushing the planes of its slab: the reference's records"""
    import threading
    from ftk_amd import tslab, _lib
    L = _lib.load()
    g = load_golden("random_2d_vector_23x20x5")
    world, nt = 2, len(g["steps"])
    hub = L.ftkx_slab_hub_create(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            tr = vector_tracker(gpu, g)
            tr.initialize()
            tr.set_slab_hub(hub, r, nt)
            t0, t1 = tslab.slab_range(nt, world, r)
            for k, t in enumerate(range(t0, t1)):
                tr.push_vector_field_components(planes_of(g["steps"][t]))
                if k:
                    tr.advance_timestep()
                if t == t1 - 1:
                    tr.update_timestep()
            tr.finalize()
            out[r] = tr.get_critical_points()
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
    assert_records_equal(points_as_fixture(out[0]), g["records"], coord_tol=0.0, what="two slab ranks, components (bit-exact)")


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu, meshes):
    import torch
    E, U = gpu._lib.E_INVALID, gpu._lib.E_UNSUPPORTED
    m = meshes["gyre2d"]
    V, nt = m["V"], len(m["V"])
    n = V[0].shape[0] * V[0].shape[1]
    ctx = vector_context(gpu, m["dims"])
    L, h = ctx._L, ctx._h

    def refused(code, call):
        with pytest.raises(gpu.FtkxError) as e:
            call()
        assert e.value.code == code, str(e.value)

    def good_push(t):
        ctx.push_slice_planar(t, components(V[t], np.float64, "separate", 0))

    three = np.zeros((3,) + V[0].shape[:2])
    refused(E, lambda: ctx.push_slice_planar(0, three))                                                   # wrong nc
    refused(E, lambda: ctx.temporal_push_planar(three))                                                   # (the filter is off as well)
    good_push(0)
    a = torch.zeros(n + 8, dtype=torch.float64, device="cuda"); b = torch.zeros(n + 8, dtype=torch.float64, device="cuda")
    d = torch.zeros(2 * n + 8, dtype=torch.float64, device="cuda")
    p, q, r = a.data_ptr(), b.data_ptr(), d.data_ptr()
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)      # noqa: E731
    assert L.ftkx_push_slice_planar(h, 1, ptrs(p, None), 2, None, None, 1) == E                           # a null plane
    assert L.ftkx_push_slice_planar(h, 1, None, 2, None, None, 1) == E
    assert L.ftkx_push_slice_planar(h, 1, ptrs(p, q + 4), 2, None, None, 1) == E                          # a misaligned plane
    assert L.ftkx_push_slice_planar_f32(h, 1, ptrs(p, q + 2), 2, None, None, 1) == E
    assert L.ftkx_push_slice_planar(h, 1, ptrs(p, q), 2, None, None, 3) == E                              # on_device
    good_push(1)
    before = ctx.planar_counts()
    refused(E, lambda: ctx.concat([p, None], 8, r))
    refused(E, lambda: ctx.concat([p], 8, r)); refused(E, lambda: ctx.concat([p, q, p, q], 8, r))        # nc 2 or 3
    refused(E, lambda: ctx.concat([p, q], 0, r)); refused(E, lambda: ctx.concat([p, q], 8, None))
    refused(E, lambda: ctx.concat([p + 4, q], 8, r)); refused(E, lambda: ctx.concat([p + 2, q], 8, r, f32=True))      # misaligned planes
    refused(E, lambda: ctx.concat([p, q], 8, r + 4))                                                      # misaligned dst
    refused(E, lambda: ctx.concat([p, q], 8, p)); refused(E, lambda: ctx.concat([p, q], 8, q - 8 * 15))   # dst overlapping a plane: its start, its end
    refused(E, lambda: ctx.concat([r + 8 * 15, q], 8, r))
    ms = (C.c_double * 2)()
    assert L.ftkx_debug_concat_relaunch(h, ptrs(p, q), 2, 0, 8, r, 0, ms) == E and L.ftkx_debug_concat_relaunch(h, ptrs(p, q), 2, 0, 8, r, 2, None) == E
    assert ctx.planar_counts() == before                                                                  # none of these launched anything
    ctx.concat([p, p], 8, r)                                                                              # planes may be one another
    assert len(ctx.debug_concat_relaunch([p, q], 8, r, 2)) == 2
    assert ctx.planar_counts() == (before[0] + 3, before[1])
    # settings that take no vector slices, or no J beside V
    ctx.set_spatial_smoothing(1.0, 3)
    refused(U, lambda: good_push(2))
    ctx.set_spatial_smoothing(1.0, 0)
    ctx.set_clamp(-1e300, 1e300)
    refused(U, lambda: ctx.push_slice_planar(2, components(V[2], np.float64, "separate", 0), m["J"][2], None))
    ctx.set_clamp()
    for t in range(2, nt):
        good_push(t)
    recs, factors = sweep_steps(gpu, ctx, range(nt))
    assert factors == m["plain"][1] and same_records(recs, m["plain"][0])
    ctx.close()
    # what Python refuses before any call into the library
    c2 = vector_context(gpu, m["dims"])
    u, v = np.zeros(V[0].shape[:2]), np.zeros(V[0].shape[:2], dtype=np.float32)
    with pytest.raises(TypeError):
        c2.push_slice_planar(0, [u, v])                                                                   # a mix of dtypes
    with pytest.raises(ValueError):
        c2.push_slice_planar(0, [u, torch.zeros(V[0].shape[:2], dtype=torch.float64, device="cuda")])     # a mix of host and device
    with pytest.raises(ValueError):
        c2.push_slice_planar(0, np.zeros((2, V[0].shape[0], 2 * V[0].shape[1]))[:, :, ::2])                   # not contiguous
    with pytest.raises(TypeError):
        c2.push_slice_planar(0, [u.astype(np.int64), u.astype(np.int64)])
    assert c2.planar_counts() == (0, 0)
    c2.close()
    # a multi-device tracker takes the interleaved FP64 array only
    g = load_golden("random_2d_vector_23x20x5")
    tr = vector_tracker(gpu, g, device_ids=[0, 0])
    tr.initialize()
    with pytest.raises(gpu.FtkxError) as e:
        tr.push_vector_field_components(planes_of(g["steps"][0]))
    assert e.value.code == U
    tr.push_vector_field_snapshot(g["steps"][0]); tr.push_vector_field_snapshot(g["steps"][1])
    tr.advance_timestep(); tr.update_timestep()
    tr.close()
    # ... and a single-device one refuses planes that are not its dimension's, then goes on
    tr = vector_tracker(gpu, g)
    tr.initialize()
    with pytest.raises(gpu.FtkxError) as e:
        tr.push_vector_field_components(planes_of(g["steps"][0]) + planes_of(g["steps"][0])[:1])
    assert e.value.code == E
    tr.close()
