"""Every path of the sweep on meshes whose array lattice begins at (5, 7[, 3]) and whose core lies strictly inside the domain
(tests/mesh_cases.py; shown sound without a GPU in tests/test_mesh_cases.py), against the oracle on the same (domain, core, array lattice),
bit for bit: the host-driven batch under every mask kernel family and summary geometry, the series pass in its three forms, the integer
regime through the tile kernel, the drop-in boundary, the trackers (one context, two, image bounds, rectilinear coordinates), aux sampling
behind a batch and inside a pass, and the patch kernels.  Each test asserts that the path it means was the path taken.

Every other mesh of the suite but one has the array lattice at 0 and core = domain: there a dropped `- m.ext_st[d]`, or a core taken for
the domain, changes nothing."""
import numpy as np
import pytest

import mesh_cases as M
import one_launch_cases as K
import sample_cases as SC
from common import assert_records_equal
from halo_cases import patch_addresses

pytestmark = pytest.mark.gpu

NAMES = [f"{M._label(s[0], s[1])}_{p}" for s in M.SHAPES for p in ("ragged", "aligned")] + ["3d_scalar_40x21x11_huge"]
SUMMARY = [f"{M._label(s[0], s[1])}_{p}" for s in M.SHAPES if s[5] for p in ("ragged", "aligned")]
MASKS_INVALID, NOT_DEVICE_DRIVEN = 2, 1 | 2 | 4 | 8      # (sweep_params.hpp: SERIES_*; the second: the statuses after which the host-driven batch sweeps the steps)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


@pytest.fixture(scope="module")
def cases(oracle):
    return M.cases()


def _ctx(gpu, c, **opts):
    ctx = gpu.Context(c.nd)
    ctx.set_mesh(c.dom, c.core, c.ext)
    o = dict(jacobian_symmetric=int(c.nv == 1), derive_jacobian=1, tag_mode=c.tag_mode)
    if c.bounds is not None:
        o["coords_bounds"] = c.bounds
    o.update(opts)
    ctx.set_options(**o)
    return ctx


def _push(ctx, c):
    for t, a in c.slices().items():
        (ctx.push_scalar_slice if c.nv == 1 else ctx.push_slice)(t, a)


def _as_fixture(recs):
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = recs["aux"] & 1
    out["timestep"] = recs["aux"] >> 1
    return out


def _assert_reference(recs, factors, c, what, in_order=True):
    ref, rf, _ = M.reference(c)
    assert [int(v) for v in factors] == rf, (what, list(factors), rf)
    assert len(recs) == len(ref), f"{what}: {len(recs)} records, expected {len(ref)}"
    if in_order:
        bad = np.flatnonzero(recs["tag"] != ref["tag"])
        assert bad.size == 0, f"{what}: {bad.size} records out of tag order, the first at {int(bad[0])} of {len(ref)}"
    assert_records_equal(_as_fixture(recs), ref, coord_tol=0.0, what=what)


def _last_mask_kernel(ctx):
    return (ctx._L.ftkx_last_mask_kernel() or b"").decode()


def _context_run(gpu, c, mode, dom, core, ext):
    """test_gpu_fuzz._context_run on a mesh of the caller's: the host-driven batch behind the exact pre-pass ("exact_prepass"), behind the
    one-pass prepare ("one_pass"), and announced first ("announced") -> (records, factors, statistics, the mask kernel launched last)"""
    from ftk_amd import tslab
    scalar = c.nv == 1
    ctx = gpu.Context(c.nd)
    ctx.set_mesh(dom, core, ext)
    ctx.set_options(jacobian_symmetric=int(scalar), derive_jacobian=1, tag_mode=int(c.tag_mode))
    _push(ctx, c)
    nt = len(c.slice_ts)
    assert c.slice_ts == list(range(nt)) and list(c.ts) == list(range(c.n))
    # (the slices are those of the steps: the last step is ordinal, so there are as many)
    if mode == "exact_prepass":
        res = [ctx.slice_resolution(t)[0] for t in range(nt)]
    else:
        if mode == "announced":
            ctx.sweep_announce(c.ts, c.scopes)
        rm = ctx.slices_prepare(range(nt), 0)
        res = [rm[t][0] for t in range(nt)]
    factors = tslab.factors_from_resolutions(res)[:c.n]
    ctx.sweep_enqueue_many(c.ts, c.scopes, factors)
    recs = ctx.sweep_collect()
    st, name = ctx.stats(), _last_mask_kernel(ctx)
    ctx.close()
    return recs, factors, st, name


def _assert_cull(c, st, what):
    """the cull is on, keeps cells and drops cells -- never more than the strict-sign rule allows (mesh_cases.cull_counts)"""
    cells, removable = M.cull_counts(c)
    print(what, "cells", st["cells"], "survived", st["cells_survived"], "removable", removable, "tested", st["simplices_tested"], "of", st["work_items"])
    assert st["cull_enabled"] == 1 and st["cells"] == cells, (what, st)
    assert cells - removable <= st["cells_survived"], (what, st, removable)
    if c.kind == "huge":
        assert st["cells_survived"] == cells, (what, st)
    else:
        assert 0 < st["cells_survived"] < cells, (what, st)


# ---- the host-driven batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_driven_batch(gpu, cases, name, monkeypatch):
    c = cases[name]
    if c.mask_plan:
        monkeypatch.setenv("FTKX_MASK_PLAN", c.mask_plan)
    for mode in ("exact_prepass", "one_pass", "announced"):
        what = f"{name} [{mode}]"
        recs, factors, st, kernel = _context_run(gpu, c, mode, c.dom, c.core, c.ext)
        assert kernel == c.family, (what, kernel)
        _assert_reference(recs, factors, c, what)
        _assert_cull(c, st, what)


@pytest.mark.parametrize("name", SUMMARY)
def test_host_driven_batch_under_every_summary_geometry(gpu, cases, name, monkeypatch):
    """FTKX_U_ROWS: -1 no summaries (the one-level cull on the core's words), 1 a summary byte per word of 8, 4 per 8 x 4 block (3D; the
    default there is 8 x 16): coarse_view's floor of the core's first word and row, the refine kernel's rows at the core's edge"""
    c = cases[name]
    if c.mask_plan:
        monkeypatch.setenv("FTKX_MASK_PLAN", c.mask_plan)
    survived = {}
    for rows in ("-1", "1") + (("4",) if c.nd == 3 else ()):
        monkeypatch.setenv("FTKX_U_ROWS", rows)
        what = f"{name} [one_pass, FTKX_U_ROWS={rows}]"
        recs, factors, st, kernel = _context_run(gpu, c, "one_pass", c.dom, c.core, c.ext)
        # (mask_vec2_kernel is the vector kernel WITH block summaries: without them, or with one per word, plan_masks takes mask_vec_kernel)
        family, summaries = M.planned(c, rows)
        assert kernel == family and summaries == (rows != "-1"), (what, kernel, family, summaries)
        _assert_reference(recs, factors, c, what)
        _assert_cull(c, st, what)
        survived[rows] = st["cells_survived"]
    # a summary stands in for mask words that were not written, with no more sign bits than the word has: it can only let more cells through
    assert survived["-1"] == min(survived.values()), survived


# ---- ftkx_sweep_series -----------------------------------------------------------------------------------------------------------------------
def _series(gpu, c, **opts):
    ctx = _ctx(gpu, c, **opts)
    _push(ctx, c)
    recs, f, _ = ctx.sweep_series(c.ts, c.scopes)
    recs = recs.copy()
    path, status = ctx.series_last_path()
    st = ctx.stats()
    ctx.close()
    return recs, f, path, status, st


@pytest.mark.parametrize("name", NAMES)
def test_series_pass_in_its_three_forms(gpu, cases, name, monkeypatch):
    c = cases[name]
    if c.mask_plan:
        monkeypatch.setenv("FTKX_MASK_PLAN", c.mask_plan)
    # as it comes: one_plan takes every case, and the launch -- which tests every simplex of the core itself, with no masks -- completes it
    # where no workgroup parks more than kOneKeys keys (ten of the cases, the one in the overflow regime among them)
    recs, f, path, status, _ = _series(gpu, c)
    print(name, "as it comes: path", path, "status", status, "one_plan", c.plan())
    _assert_reference(recs, f, c, f"{name} [series]")
    fullest = int(K.parked(c)[0].max())
    assert c.plan()["eligible"]
    if fullest <= K.limits()["kOneKeys"]:
        assert path == 4 and not (status & NOT_DEVICE_DRIVEN), (name, path, status, fullest)
    else:               # the launch finds a workgroup's key store too small and says so: the host-driven batch sweeps the steps
        assert path == 0 and (status & NOT_DEVICE_DRIVEN) == K.limits()["SERIES_OVERFLOW"], (name, path, status, fullest)
    # the kernel chain
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0")
    recs, f, path, status, _ = _series(gpu, c)
    print(name, "one=0: path", path, "status", status)
    _assert_reference(recs, f, c, f"{name} [series, one=0]")
    if M.masks_need_the_vertex_rule(c):      # (the huge case and three rough 3D ones: a quantised component of safe_m and more under a factor of 2^19 .. 2^21)
        assert path == 0 and (status & NOT_DEVICE_DRIVEN) == MASKS_INVALID, (name, path, status)
        return
    assert path in (1, 2) and not (status & NOT_DEVICE_DRIVEN), (name, path, status)
    assert (gpu._lib.load().ftkx_last_mask_kernel() or b"").decode() == c.family      # (the pass just completed launched the mask kernel last in this process)
    # the split pass: two passes in flight, the second next to the tail of the first
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,split=2")
    ctx = _ctx(gpu, c)
    _push(ctx, c)
    recs, f, _ = ctx.sweep_series(c.ts, c.scopes)                   # (not pipelined: in order; the passes behind it know the record count)
    assert ctx.series_last_path()[0] in (1, 2)
    _assert_reference(recs.copy(), f, c, f"{name} [series, split=2, the plain pass]")
    ctx.invalidate_masks()
    ctx.sweep_series_submit(c.ts, c.scopes)
    ctx.invalidate_masks()
    ctx.sweep_series_submit(c.ts, c.scopes)
    for k in range(2):
        recs, f, _ = ctx.sweep_series_complete()
        path, status = ctx.series_last_path()
        print(name, "split=2, pass", k, ": path", path, "status", status)
        assert path == 5 and not (status & NOT_DEVICE_DRIVEN), (name, k, path, status)
        _assert_reference(recs.copy(), f, c, f"{name} [series, split, pass {k}]")
    ctx.close()


# ---- the integer regime: the tile kernel ---------------------------------------------------------------------------------------------------------
TILE = ["2d_scalar_40x23_ragged", "2d_vector_40x23_aligned", "2d_scalar_136x21_aligned", "3d_scalar_40x21x11_aligned", "3d_scalar_42x19x9_ragged", "3d_vector_24x13x9_ragged",
        "3d_vector_25x13x9_aligned", "3d_scalar_40x21x11_huge"]


@pytest.mark.parametrize("fan", ["0", "1", "2"])
@pytest.mark.parametrize("name", TILE)
def test_exact_only_takes_the_tile_kernel(gpu, cases, name, fan, monkeypatch):
    """exact_only: every simplex of the core through tile_kernel -- tiles that begin at core_st, staged from the array at origin - ext_st -- in
    each form of its fan (FTKX_TILE_FAN)"""
    c = cases[name]
    monkeypatch.setenv("FTKX_TILE_FAN", fan)
    recs, f, path, status, st = _series(gpu, c, exact_only=1)
    print(name, "fan", fan, "path", path, "status", status, st)
    assert path == 0 and st["cull_enabled"] == 0, (name, fan, path, status, st)
    assert st["simplices_tested"] > 0.5 * st["work_items"], (name, fan, st)
    _assert_reference(recs, f, c, f"{name} [exact_only, FTKX_TILE_FAN={fan}]")


def test_overflow_regime_keeps_every_cell(gpu, cases):
    """the `huge` case without exact_only: every quantised component is beyond safe_m, no vertex carries a sign, the cull is on and drops
    nothing -- all the core's cells reach the integer test, whose wrapped determinants are the reference's answer"""
    c = cases["3d_scalar_40x21x11_huge"]
    recs, factors, st, kernel = _context_run(gpu, c, "one_pass", c.dom, c.core, c.ext)
    _assert_reference(recs, factors, c, "huge [one_pass]")
    _assert_cull(c, st, "huge [one_pass]")
    assert kernel == c.family and st["simplices_tested"] > 0.5 * st["work_items"], (kernel, st)


# ---- the drop-in boundary --------------------------------------------------------------------------------------------------------------------
BOUNDARY = ["2d_scalar_40x23_ragged", "2d_vector_40x23_aligned", "2d_scalar_41x23_aligned", "3d_scalar_42x19x9_ragged", "3d_vector_24x13x9_aligned"]


def _given_fields(oracle, c):
    """(V, J, S) of slices 0 and 1, derived by the oracle: the boundary takes them as the reference's trackers hand them over"""
    return [M.derived(c, c.slices()[k]) for k in (0, 1)]


@pytest.mark.parametrize("name", BOUNDARY)
def test_boundary_call_with_an_origin(gpu, oracle, cases, name):
    c = cases[name]
    nd = c.nd
    fields = _given_fields(oracle, c)
    factor = M.reference(c)[1][0]
    t = 3                                              # the current timestep of the call: not 0
    f = gpu.extract_cp2dt if nd == 2 else gpu.extract_cp3dt
    for scope in (gpu.SCOPE_ORDINAL, gpu.SCOPE_INTERVAL):
        nxt = scope == gpu.SCOPE_INTERVAL
        for tag_mode in (oracle.TAG_WORK_INDEX, oracle.TAG_REFERENCE, oracle.TAG_EXACT64):
            what = f"{name} scope {scope} tag mode {tag_mode}"
            ref = oracle.sweep(nd, scope, t, c.dom, c.core, c.ext, (fields[0][0], fields[1][0]), (fields[0][1], fields[1][1]),
                               (fields[0][2], fields[1][2]) if c.nv == 1 else None, factor, jacobian_symmetric=(c.nv == 1), tag_mode=tag_mode, nthreads=4)
            assert len(ref) >= 20, what
            opt = gpu.default_options(jacobian_symmetric=int(c.nv == 1), tag_mode=tag_mode)
            got = f(scope, t, (list(c.dom[0]) + [0], list(c.dom[1]) + [2 ** 31 - 1]), (list(c.core[0]) + [t], list(c.core[1]) + [1]), c.ext,
                    fields[0][0], fields[1][0] if nxt else None, fields[0][1], fields[1][1] if nxt else None,
                    fields[0][2], fields[1][2] if nxt else None, factor, opt)
            refr = np.zeros(len(ref), dtype=got.dtype)
            for fld in ("x", "t", "scalar", "type", "tag"):
                refr[fld] = ref[fld]
            assert_records_equal(got, refr, coord_tol=0.0, what=what)


def test_boundary_refuses_explicit_coordinates_with_an_origin(gpu, oracle, cases):
    """the boundary's `coords` array lies over `ext` and is read at the lattice coordinate: with an origin the call is refused, nothing runs"""
    c = cases["2d_scalar_40x23_ragged"]
    fields = _given_fields(oracle, c)
    coords = np.zeros((c.dims[1], c.dims[0], 2))
    args = (gpu.SCOPE_ORDINAL, 0, (list(c.dom[0]) + [0], list(c.dom[1]) + [2 ** 31 - 1]), (list(c.core[0]) + [0], list(c.core[1]) + [1]))
    with pytest.raises(gpu.FtkxError) as e:
        gpu.extract_cp2dt(*args, c.ext, fields[0][0], None, fields[0][1], None, fields[0][2], None, 256, None, coords=coords)
    assert e.value.code == gpu._lib.E_UNSUPPORTED, e.value
    # (the same call with the array lattice at 0 is taken)
    z = M.at_origin_zero(c)
    args = (gpu.SCOPE_ORDINAL, 0, (list(z.dom[0]) + [0], list(z.dom[1]) + [2 ** 31 - 1]), (list(z.core[0]) + [0], list(z.core[1]) + [1]))
    got = gpu.extract_cp2dt(*args, z.ext, fields[0][0], None, fields[0][1], None, fields[0][2], None, 256, None, coords=coords)
    assert len(got) > 0


# ---- the trackers ----------------------------------------------------------------------------------------------------------------------------
TRACKED = ["2d_scalar_40x23_ragged", "3d_scalar_42x19x9_aligned", "2d_vector_40x23_aligned", "3d_vector_24x13x9_ragged"]


def _rect(c):
    """REGULAR_COORDS_RECTILINEAR arrays, indexed by the LATTICE coordinate (sweep_device.hpp: coords_rect[d][vx]): ext_st + ext_sz entries,
    closed form as in oracle/ref_driver.cpp"""
    return [np.array([0.5 * i + 0.0625 * ((i * (d + 3)) % 5) + d for i in range(c.ext[0][d] + c.ext[1][d])]) for d in range(c.nd)]


def _track(gpu, c, **kw):
    from gpu_common import run_tracker
    steps = [c.slices()[t] for t in c.slice_ts]
    return run_tracker(steps, c.nd, c.nv, tag_mode=gpu.TAG_EXACT64, array_start=c.ext[0], **kw)


@pytest.mark.parametrize("name", TRACKED)
def test_tracker_with_an_array_origin(gpu, cases, name):
    """critical_point_tracker_regular passes array_domain.start(d) straight through as ext_st (tracker.cpp); its core is its domain"""
    c = cases[name]
    w = M.whole_domain(c)
    ref, rf, _ = M.reference(w)
    got, gf, stats = _track(gpu, c)
    assert [int(v) for v in gf] == rf, (name, list(gf), rf)
    assert_records_equal(got, ref, coord_tol=0.0, what=f"{name} [tracker]")
    # two contexts on one device, the timesteps dealt in blocks
    got, gf, _ = _track(gpu, c, device_ids=[0, 0], block=1, factor_each_step=False)
    assert int(gf[-1]) == rf[-1]
    assert_records_equal(got, ref, coord_tol=0.0, what=f"{name} [tracker, two contexts]")
    # a domain of the caller's: the case's core
    inner = M.whole_domain(c)
    inner.name, inner.dom, inner.core = c.name + "@inner", c.core, c.core
    iref, irf, _ = M.reference(inner)
    got, gf, _ = _track(gpu, c, domain=c.core)
    assert [int(v) for v in gf] == irf and 0 < len(iref) < len(ref)
    assert_records_equal(got, iref, coord_tol=0.0, what=f"{name} [tracker, domain = the case's core]")


@pytest.mark.parametrize("name", TRACKED[:2])
def test_tracker_coordinates_with_an_array_origin(gpu, oracle, cases, name):
    """image bounds: the device divides (v - ext_st) by ext_sz - 1; rectilinear: arrays indexed by the lattice coordinate itself, which
    must reach the domain's last vertex -- one entry short is FTKX_E_INVALID before anything is launched"""
    c = cases[name]
    bounds = [-1.5, 2.25, 10.0, 11.5, 100.0, 130.0][:2 * c.nd]
    w = M.whole_domain(c)
    w.name, w.bounds = c.name + "@whole@bounds", bounds
    ref, rf, _ = M.reference(w)
    got, gf, _ = _track(gpu, c, bounds=bounds)
    assert [int(v) for v in gf] == rf
    assert_records_equal(got, ref, coord_tol=0.0, what=f"{name} [tracker, bounds]")
    plain, _, _ = M.reference(M.whole_domain(c))
    assert not np.array_equal(ref["x"], plain["x"]) and np.array_equal(ref["tag"], plain["tag"])
    # rectilinear
    rect = _rect(c)
    rref = M.reference_rectilinear(M.whole_domain(c), rect)
    got, gf, _ = _track(gpu, c, rectilinear=rect)
    assert [int(v) for v in gf] == rf
    assert_records_equal(got, rref, coord_tol=0.0, what=f"{name} [tracker, rectilinear]")
    assert not np.array_equal(rref["x"], plain["x"])
    # arrays that stop one entry before the domain's last vertex
    last = [w.dom[0][d] + w.dom[1][d] - 1 for d in range(c.nd)]
    for d in range(c.nd):
        short = [r if k != d else r[:last[d]] for k, r in enumerate(rect)]
        with pytest.raises(gpu.FtkxError) as e:
            _track(gpu, c, rectilinear=short)
        assert e.value.code == gpu._lib.E_INVALID, (d, e.value)
        enough = [r if k != d else r[:last[d] + 1] for k, r in enumerate(rect)]
        got, _, _ = _track(gpu, c, rectilinear=enough)
        assert_records_equal(got, rref, coord_tol=0.0, what=f"{name} [tracker, rectilinear, axis {d} as short as it may be]")


# ---- aux sampling ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_scalar_40x23_ragged", "3d_scalar_42x19x9_aligned"])
def test_aux_fields_sampled_with_an_array_origin(gpu, cases, name, monkeypatch):
    c = cases[name]
    e1, e2 = M.aux_expected(c, 0), M.aux_expected(c, 1)
    ref, _, _ = M.reference(c)

    def armed_context():
        ctx = _ctx(gpu, c)
        _push(ctx, c)
        for t in c.slice_ts:
            ctx.push_aux_slice(t, 1, M.aux_field(c, t, 0)); ctx.push_aux_slice(t, 2, M.aux_field(c, t, 1))
        return ctx

    def check(recs, what):
        assert np.array_equal(recs["tag"], ref["tag"]), what
        assert SC.same_doubles(recs["scalar"][:, 0], ref["scalar"][:, 0]), what
        for slot, e in ((1, e1), (2, e2)):
            bad = int((np.ascontiguousarray(recs["scalar"][:, slot]).view(np.uint64) != e.view(np.uint64)).sum())
            assert SC.same_doubles(recs["scalar"][:, slot], e), f"{what}: {bad} of {len(e)} values of scalar[{slot}] differ from the oracle's"
    # behind a host-driven batch: ftkx_sample_aux
    ctx = armed_context()
    ctx.sweep_enqueue_many(c.ts, c.scopes, M.reference(c)[1])
    recs = np.array(ctx.sweep_collect())
    assert not recs["scalar"][:, 1:].view(np.uint64).any()
    ctx.sample_aux(recs)
    assert ctx.sample_counts() == (1, len(recs))
    check(recs, f"{name} [sample_aux behind a batch]")
    ctx.close()
    # inside a series pass (the kernel chain): ftkx_set_series_sampling
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0")
    ctx = armed_context()
    ctx.set_series_sampling(True)
    recs, f, _ = ctx.sweep_series(c.ts, c.scopes)
    recs = recs.copy()
    path, _ = ctx.series_last_path()
    assert ctx.series_sampled() == (3, 1) and path in (1, 2), (ctx.series_sampled(), path)
    assert ctx.series_sample_counts()[:2] == (1, len(recs)) and ctx.sample_counts() == (0, 0)
    check(recs, f"{name} [sampled inside the pass]")
    ctx.close()


# ---- the patch kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_scalar_40x23_ragged", "3d_scalar_40x21x11_aligned", "2d_vector_40x23_ragged"])
def test_patches_round_trip_with_an_array_origin(gpu, cases, name):
    """ftkx_gather_patches on the owner of a slice gives, per cell of the core, the array values at corner - ext_st - 2 .. + 3 on every axis
    (clamped to the array); ftkx_scatter_patches into a masked halo slice -- a zeroed array -- changes exactly those elements"""
    import torch
    c = cases[name]
    nd, ncomp, dims = c.nd, (1 if c.nv == 1 else c.nd), c.dims
    dev = torch.device("cuda", 0)
    a = c.slices()[1]
    flat = a.reshape(-1, ncomp)
    ncell = c.cells

    def push(ctx, t, arr):
        (ctx.push_scalar_slice if c.nv == 1 else ctx.push_slice)(t, arr)

    def where(cells):
        """array index (flat, x fastest) of every element of every cell's patch"""
        return patch_addresses(c, cells)
    B = _ctx(gpu, c)
    push(B, 1, a)
    assert B.patch_doubles() == 6 ** nd * ncomp
    # the first and the last cell of the core, cells in its first and last word, some in between
    rng = np.random.default_rng(5)
    picked = np.unique(np.concatenate([[0, 1, c.core[1][0] - 1, c.core[1][0], ncell - c.core[1][0], ncell - 1], rng.integers(0, ncell, size=40)]))
    cells = torch.from_numpy(picked.astype(np.int64)).to(dev)
    got = B.gather_patches(1, cells, torch).cpu().numpy().reshape(len(picked), 6 ** nd, ncomp)
    at = where(picked)
    assert np.array_equal(got, flat[at]), f"{name}: gathered patches are not the array's values at cell - ext_st"
    # the receiver: slice 0 its own, slice 1 as masks only
    rm = B.slices_prepare([1], 0)
    nbytes, _cap = B.packed_masks_bytes()
    assert nbytes > 0
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    B.export_masks_packed(1, buf)
    A = _ctx(gpu, c)
    push(A, 0, c.slices()[0])
    A.slices_prepare([0], 0)
    A.push_masked_slice_packed(1, c.nv == 1, buf, 256, rm[1][1])
    everything = torch.arange(ncell, dtype=torch.int64, device=dev)
    all_at = where(np.arange(ncell))
    before = A.gather_patches(1, everything, torch).cpu().numpy().reshape(ncell, 6 ** nd, ncomp)
    assert not before.any()
    modified = torch.from_numpy(np.ascontiguousarray(got + 1000.0)).to(dev).reshape(-1)
    A.scatter_patches(1, cells, modified)
    after = A.gather_patches(1, everything, torch).cpu().numpy().reshape(ncell, 6 ** nd, ncomp)
    want = np.zeros_like(flat)
    want[at.ravel()] = flat[at.ravel()] + 1000.0
    assert np.array_equal(after, want[all_at]), f"{name}: the scatter changed other elements than its patches', or not those"
    assert 0 < len(np.unique(at)) < len(np.unique(all_at))
    A.close(); B.close()
