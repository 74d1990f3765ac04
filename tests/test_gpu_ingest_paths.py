"""The executor of ftk_amd/csrc/ingest.hip held to the plan of ingest_steps.hpp: every way an array can be pushed -- float32 / float64;
a scalar array, an interleaved vector array, component planes; host memory, this device's memory borrowed (1) or copied (2); spatial
smoothing (scalar only), perturbation and clamp on or off -- leaves the resident array the numpy pipeline of the other GPU tests gives, bit
for bit, moves exactly the debug counters the host build of the plan names, and hands its pooled staging array back.  Then the slab's own
push of a halo slice that has been processed already."""
import ctypes as C

import numpy as np
import pytest

import adjust_cases as AC
import conv_cases as CC
import ingest_cases as IC
from test_gpu_temporal import Mesh, bits

pytestmark = pytest.mark.gpu

SIGMA, SEED, CLAMP = 0.05, 2024, (-0.97, 0.96)
MESHES = [(9, 33), (5, 6, 7)]          # x first: rows of 9 and of 5 values -- pairs and 16-byte bodies meet a tail; more than one tile of the convolution


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    AC.host(); IC.host()
    return ftk_amd


def pipeline(a, t, smooth_w, adjust):
    """widen -> conv restatement -> host adjust, as the stream orders them (a vector array: adjusted by its flat index)"""
    x = np.ascontiguousarray(a).astype(np.float64)
    if smooth_w is not None:
        x = CC.conv(x, smooth_w)
    return AC.host_adjust(x, SIGMA, SEED, t, CLAMP) if adjust else x


def push(ctx, form, t, a, on_device):
    """a (numpy, its own dtype; a vector array: components last) pushed as `form`; -> the device tensors handed over (empty: host memory)"""
    import torch
    if form == "planar":
        src = [np.ascontiguousarray(a[..., k]) for k in range(a.shape[-1])]
    else:
        src = [np.ascontiguousarray(a)]
    if on_device:
        src = [torch.from_numpy(p).cuda() for p in src]
        before = [p.clone() for p in src]
        torch.cuda.synchronize()
    if form == "scalar":
        ctx.push_scalar_slice(t, src[0], on_device=on_device if on_device else None)
    elif form == "planar":
        ctx.push_slice_planar(t, src, on_device=on_device if on_device else None)
    elif on_device:          # (Context.push_slice borrows every device tensor: 2 goes to the C entry point itself)
        f = ctx._L.ftkx_push_slice_f32 if a.dtype == np.float32 else ctx._L.ftkx_push_slice
        ctx._ck(f(ctx._h, t, src[0].data_ptr(), None, None, on_device))
    else:
        ctx.push_slice(t, src[0])
    if not on_device:
        return []
    it = torch.int32 if a.dtype == np.float32 else torch.int64
    assert all(torch.equal(p.view(it), q.view(it)) for p, q in zip(src, before)), "a pushed tensor was written"
    return src


@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
@pytest.mark.parametrize("dims", MESHES, ids=["2d_9x33", "3d_5x6x7"])
def test_every_push_takes_the_path_the_plan_names(gpu, dims, vector):
    import torch
    mesh = Mesh(gpu, dims, vector)
    ctx, nd = mesh.ctx, len(dims)
    shape = tuple(reversed(dims)) + ((nd,) if vector else ())
    raw = CC.random_input(shape, 400 + nd + int(vector))
    w = gpu.gaussian_kernel(nd, 1.0, 3)
    t, pushes = 0, 0
    for form in (("interleaved", "planar") if vector else ("scalar",)):
        for smooth in ((False,) if vector else (False, True)):
            ctx.set_spatial_smoothing(1.0, 3 if smooth else 0)
            for adjust in (False, True):
                ctx.set_perturbation(SIGMA if adjust else 0.0, SEED)
                ctx.set_clamp(*(CLAMP if adjust else (None, None)))
                for dtype in (np.float64, np.float32):
                    for on_device in (0, 1, 2):
                        t += 1
                        case = (dims, form, smooth, adjust, dtype.__name__, on_device)
                        f32, planar = dtype == np.float32, form == "planar"
                        p = IC.plan(f32, planar, smooth, adjust, on_device, on_device != 0)      # (every device source lies on the context's device)
                        a = raw.astype(dtype)
                        before = (ctx.adjust_counts(), ctx.f32_counts(), ctx.planar_counts(), ctx.array_counts())
                        src = push(ctx, form, t, a, on_device)
                        after = (ctx.adjust_counts(), ctx.f32_counts(), ctx.planar_counts(), ctx.array_counts())
                        if not p.adopt:          # the context owns what it keeps: the source is overwritten at once
                            for x in src:
                                x.fill_(777.0)
                            torch.cuda.synchronize()
                        got = mesh.read(t)
                        exp = pipeline(a, t, w if smooth else None, adjust)
                        assert np.array_equal(bits(got).reshape(-1), bits(exp).reshape(-1)), case
                        # the counters the plan names, and no other
                        delta = [[x - y for x, y in zip(after[k], before[k])] for k in range(3)]
                        assert delta[0] == [int(n in p.counters) for n in ("from_float", "in_place", "out_of_place")], (case, p, delta)
                        assert delta[1] == [int(n in p.counters) for n in ("f32_widened", "f32_direct")], (case, p, delta)
                        assert sum(delta[2]) == int("planar" in p.counters) and min(delta[2]) >= 0, (case, p, delta)
                        # field arrays: dst is taken unless the source is adopted; a pooled stage is taken behind it and is back in the pool
                        # when the push returns (what the pool could not give was allocated)
                        allocated = after[3][0][0] - before[3][0][0]
                        taken = int(not p.adopt) + int(p.stage == "pooled")
                        assert after[3][1][0] - before[3][1][0] == allocated - taken + int(p.stage == "pooled"), (case, p, before[3], after[3])
                        assert after[3][0][1:] == before[3][0][1:], case                        # (no mask or summary array: nothing was swept)
                        ctx.drop_slice(t)
                        assert ctx.array_counts()[1][0] == after[3][1][0] + int(not p.adopt), case      # dst went to the pool, a borrowed array did not
                        pushes += 1
    assert pushes == 24
    # every array of this context has one size: one dst and one pooled stage were ever allocated
    assert ctx.array_counts()[0][0] == 2, ctx.array_counts()
    mesh.close()


def test_slab_halo_is_borrowed_as_it_is_and_the_settings_stay(gpu, monkeypatch):
    """The library's own push of the upper neighbour's first slice (slab.cpp, the whole-slice recovery -> ingest.hip, adopt_resident_slice)
    is not exported, so it is driven as tests/test_gpu_slab_host.py drives it: one rank that is its own upper neighbour (a series periodic
    in time) over RCCL, with a request too small for the survivors.  With smoothing, perturbation and clamp ALL set, the halo -- slice 0,
    processed when it was pushed -- must arrive unprocessed a second time: the records are those of a plain context that was pushed the
    host-processed arrays, slice nt being slice 0's very bits.  And a push behind it is processed as before: the settings are as they were."""
    import torch
    from ftk_amd import tslab, _lib
    L = _lib.load()
    monkeypatch.setenv("FTKX_DIST_CELLS", "1")
    dims, nt = (40, 33), 4
    two = [CC.random_input((33, 40), 900 + k) for k in range(2)]
    smooth0 = CC.conv(CC.conv(two[0], gpu.gaussian_kernel(2, 2.0, 5)), gpu.gaussian_kernel(2, 2.0, 5))      # (a field with structure, a little noise on top)
    steps = [np.ascontiguousarray(smooth0 * (1.0 + 0.2 * np.cos(2 * np.pi * k / nt)) + 0.01 * two[1]) for k in range(nt)]
    w = gpu.gaussian_kernel(2, 1.0, 3)
    processed = [pipeline(a, k, w, True) for k, a in enumerate(steps)]
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.set_stream(st)
    try:
        one = Mesh(gpu, dims, False)
        one.ctx.set_stream(st.cuda_stream)
        for k in range(nt + 1):
            one.ctx.push_scalar_slice(k, processed[k % nt])
        want, wf, wrun = one.ctx.sweep_series(range(nt), [gpu.SCOPE_BOTH] * nt, copy=True)
        one.close()
        assert len(want) > 0
        mesh = Mesh(gpu, dims, False)
        ctx = mesh.ctx
        ctx.set_stream(st.cuda_stream)
        ctx.set_spatial_smoothing(1.0, 3); ctx.set_perturbation(SIGMA, SEED); ctx.set_clamp(*CLAMP)
        for k in range(nt):
            ctx.push_scalar_slice(k, steps[k])
        assert np.array_equal(bits(mesh.read(0)), bits(processed[0]))
        counts = (ctx.adjust_counts(), ctx.f32_counts())
        comms = []
        for _ in range(2):
            raw = (C.c_ubyte * 128)()
            _lib.check(L.ftkx_rccl_unique_id(raw))
            comm = C.c_void_p()
            _lib.check(L.ftkx_rccl_comm_create(raw, 0, 1, 0, C.byref(comm)))
            comms.append(comm)
        slab = tslab.SlabSeries.rccl(ctx, nt, 0, 1, comms[0], side_comm=comms[1], periodic=True)
        slab.submit()
        recs, f, run = slab.complete(copy=True)
        assert slab.fallbacks >= 1, "FTKX_DIST_CELLS=1 was meant to force the whole-slice recovery"
        assert [int(v) for v in f] == [int(v) for v in wf] and run == wrun
        assert recs.tobytes() == np.ascontiguousarray(want).tobytes(), (len(recs), len(want))
        assert (ctx.adjust_counts(), ctx.f32_counts()) == counts, "the halo slice went through a kernel of the chain"
        slab.close()
        for comm in comms:
            L.ftkx_rccl_comm_destroy(comm)
        # the settings are in force as before
        ctx.push_scalar_slice(nt + 2, steps[1])
        assert np.array_equal(bits(mesh.read(nt + 2)), bits(pipeline(steps[1], nt + 2, w, True)))
        mesh.close()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
