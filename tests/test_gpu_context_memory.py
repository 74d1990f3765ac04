"""The context's buffers (ftk_amd/csrc/ctx_block.hpp) on the device: every one is admitted by its own bytes, so a context serves calls whose
buffers grow, shrink and change their element size in any order exactly as a fresh context serves each of them.  The slice arrays are such
blocks too, and come out of and go back to one pool by class and bytes (ftkx_array_pool): a mesh change under an open split pass leaves
nothing of the old lattice behind, a streaming caller allocates nothing once it is under way, a lent array is never freed or pooled."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def _patches(field, dims, cells, ncomp):
    """patches_kernel (halo_kernels.hip) restated: per cell the vertices corner - 2 .. corner + 3 of every axis, clamped to the array,
    x fastest, the components of a vertex innermost.  field: (z, y, x[, component]); dims = (x, y[, z]) = core = ext, both starting at 0"""
    nd = len(dims)
    flat = np.ascontiguousarray(field).reshape(-1, ncomp)
    out = np.empty((len(cells), 6 ** nd, ncomp), dtype=np.float64)
    for i, lin in enumerate(cells):
        corner = []
        for a in range(nd):
            corner.append(int(lin) % dims[a])
            lin = int(lin) // dims[a]
        for p in range(6 ** nd):
            at, stride, q = 0, 1, p
            for a in range(nd):
                x = min(max(corner[a] - 2 + q % 6, 0), dims[a] - 1)
                q //= 6
                at += x * stride
                stride *= dims[a]
            out[i, p] = flat[at]
    return out.reshape(-1)


@pytest.mark.parametrize("dims,cells", [((12, 10), [0, 7, 59, 64, 119]), ((7, 6, 5), [0, 100, 209])])
@pytest.mark.parametrize("order", ["scalar, vector", "vector, scalar"])
def test_patch_staging_follows_component_count(gpu, dims, cells, order):
    """ftkx_gather_patches from host memory stages cells and patches through device buffers of the context.  One context holds scalar
    slices, then -- all of them dropped -- vector slices (or the other way round): the same cells then take nd times (1 / nd of) the
    patch doubles, 36 / 72 per cell in 2D and 216 / 648 in 3D.  The staging is admitted by the bytes of the patch buffer itself (it used
    to be admitted by the number of cells, and the second call overran the first call's buffer).  Cell 0 and the last cell of the mesh are
    among the cells: the clamping at both borders.  Every result equals the numpy restatement of the kernel bit for bit, with the cells
    given on the host and on the device."""
    import torch
    nd = len(dims)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    shape = tuple(reversed(dims))
    fields = {"scalar": rng.standard_normal(shape), "vector": rng.standard_normal(shape + (nd,))}
    box = ([0] * nd, list(dims))
    host_cells = torch.tensor(cells, dtype=torch.int64)
    assert cells[0] == 0 and cells[-1] == int(np.prod(dims)) - 1
    ctx = gpu.Context(nd)
    try:
        ctx.set_mesh(box, box, box)
        for kind in order.split(", "):
            ncomp = 1 if kind == "scalar" else nd
            if kind == "scalar":
                ctx.push_scalar_slice(0, fields[kind])
            else:
                ctx.push_slice(0, fields[kind])
            assert ctx.patch_doubles() == 6 ** nd * ncomp
            want = _patches(fields[kind], dims, cells, ncomp)
            got = ctx.gather_patches(0, host_cells, torch)
            assert not got.is_cuda and got.numel() == len(cells) * 6 ** nd * ncomp
            assert got.numpy().tobytes() == want.tobytes(), (kind, "cells on the host")
            got_dev = ctx.gather_patches(0, host_cells.to(dev), torch)
            assert got_dev.is_cuda and got_dev.cpu().numpy().tobytes() == want.tobytes(), (kind, "cells on the device")
            ctx.drop_slice(0)
    finally:
        ctx.close()


def _series_steps(gpu, ctx, dims, nt, keep):
    """every call that sizes a buffer of the context, over one woven series; what each of them returned, in a comparable form"""
    import torch
    from ftk_amd import synthetic, tslab
    dev = torch.device("cuda", 0)
    dom = ([2, 2], [d - 3 for d in dims])
    ctx.set_mesh(dom, dom, ([0, 0], list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_EXACT64)
    steps = [synthetic.woven(dims, k, nt, torch, dev) for k in range(nt)]
    torch.cuda.synchronize()
    keep.append(steps)
    for t in range(nt):
        ctx.push_scalar_slice(t, steps[t])
    out = {}
    out["resolution"] = np.array([ctx.slices_resolution(range(nt))[t] for t in range(nt)]).tobytes()
    rm = ctx.slices_prepare(range(nt), 0)
    out["prepare"] = np.array([rm[t] for t in range(nt)]).tobytes()
    factors = tslab.factors_from_resolutions([rm[t][0] for t in range(nt)])
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    nbytes, cap = ctx.packed_masks_bytes()
    message = None
    if nbytes:                       # the mesh has summarised masks: the last slice's, as one message in host memory
        message = torch.zeros((nbytes,), dtype=torch.uint8)
        ctx.export_masks_packed(nt - 1, message)
        h = message.numpy()
        head = h[:32].view(np.uint64)
        count, ub = int(head[0]), int(head[1])
        assert count <= cap
        off_idx = 32 + (ub + 7) // 8 * 8
        off_words = off_idx + (cap * 4 + 7) // 8 * 8
        idx, words = h[off_idx:off_idx + 4 * count].view(np.uint32), h[off_words:off_words + 8 * count].view(np.uint64)
        by_index = np.argsort(idx, kind="stable")      # (the words are appended in the order the wavefronts arrive; behind `count` nothing is written)
        out["message"] = h[:32 + ub].tobytes() + idx[by_index].tobytes() + words[by_index].tobytes()
    ctx.sweep_enqueue_many(range(nt), scopes, factors)
    recs = np.array(ctx.sweep_collect())
    assert len(recs) > 0
    out["collect"] = recs.tobytes()
    recs, f, run = ctx.sweep_series(range(nt), scopes)
    out["series"] = np.array(recs).tobytes() + np.asarray(f).tobytes() + np.float64(run).tobytes()
    if message is not None:          # the last slice again, as masks only, out of host memory; the cells its neighbour's sweep would ask for
        ctx.drop_slice(nt - 1)
        ctx.push_masked_slice_packed(nt - 1, True, message, 256, rm[nt - 1][1])
        ctx.sweep_enqueue_many(range(nt - 1), [gpu.SCOPE_BOTH] * (nt - 1), factors[:nt - 1])
        cells = ctx.sweep_cull(nt - 1, torch, torch.device("cpu")).numpy()
        ctx.sweep_cancel()
        out["cells"] = np.sort(cells).tobytes()             # (appended in the order the wavefronts arrive)
    for t in range(nt):
        ctx.drop_slice(t)
    return out


def test_one_context_grows_in_every_order(gpu):
    """Woven series of 16 x 16 x 4, 48 x 40 x 6 and 16 x 16 x 4 again on ONE context that is given a new mesh between them, and each on a
    fresh context: ftkx_slices_resolution over several slices, ftkx_slices_prepare, the batched sweep, the series pass, a packed mask
    message exported into host memory, the same message pushed from host memory as a masks-only slice and the cull against it.  Every
    buffer of the one context grows with the second series and is larger than needed in the third; records, factors, reductions,
    messages and cell lists are the same bytes either way.  (A message is compared as its header, its summary array and its (index, word)
    pairs in index order, the cell list sorted: both are appended by atomics, and nothing is written behind their counts.)"""
    series = [((16, 16), 4), ((48, 40), 6), ((16, 16), 4)]
    keep = []
    one = gpu.Context(2)
    try:
        got = [_series_steps(gpu, one, dims, nt, keep) for dims, nt in series]
    finally:
        one.close()
    for k, (dims, nt) in enumerate(series):
        fresh = gpu.Context(2)
        try:
            want = _series_steps(gpu, fresh, dims, nt, keep)
        finally:
            fresh.close()
        assert got[k].keys() == want.keys(), (k, sorted(got[k]), sorted(want))
        for name in want:
            assert got[k][name] == want[name], (k, dims, nt, name)
    assert "message" in got[1] and "cells" in got[1]          # (48 x 40 has summarised masks: the halo steps ran)
    assert got[0] == got[2]


# ---- the slice arrays: blocks, one pool by class and bytes ------------------------------------------------------------------------------------
def _context(gpu, dims):
    nd = len(dims)
    ctx = gpu.Context(nd)
    _mesh(gpu, ctx, dims)
    return ctx


def _mesh(gpu, ctx, dims, options=True):
    nd = len(dims)
    dom = ([2] * nd, [d - 3 for d in dims])
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    if options:                                                # (refused while a series pass is open; they stay as they are then)
        ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=gpu.TAG_EXACT64)


def _snapshots(dims, nt):
    """woven (2D) / a moving extremum with dyadic centre and velocity (3D), as device tensors"""
    import torch
    from ftk_amd import synthetic
    dev = torch.device("cuda", 0)
    if len(dims) == 2:
        steps = [synthetic.woven(dims, k, nt, torch, dev) for k in range(nt)]
    else:
        x0, dirv = synthetic.moving_extremum_params(dims)
        steps = [synthetic.moving_extremum(dims, k, x0, dirv, torch, dev) for k in range(nt)]
    torch.cuda.synchronize()
    return steps


def _scopes(gpu, nt):
    return [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]


def _bytes(result):
    recs, f, run = result
    return np.array(recs).tobytes() + np.asarray(f).tobytes() + np.float64(run).tobytes()


@pytest.mark.parametrize("series", [[((16, 16), 4), ((48, 40), 6), ((16, 16), 4)], [((9, 9, 9), 3), ((12, 10, 9), 3), ((9, 9, 9), 3)]], ids=["2d", "3d"])
def test_mesh_change_under_an_open_split_pass(gpu, series, monkeypatch):
    """A split pass is submitted, all its slices are dropped while it is open -- they are parked with it, not in the context's map of
    slices, which is all ftkx_set_mesh looks at -- the mesh is set to a larger lattice, and only then the pass is completed.  Before,
    the parked arrays of the old lattice then went into the pools of the new one (field arrays under the new lattice's count, mask arrays
    with no size at all) and the next push took them for the larger lattice.  Now ftkx_set_mesh waits for the pass's tail and releases what
    it parked before it clears the pool: right after it nothing is pooled, the pass's records are those of a fresh context, and so is
    every later series (the larger lattice, then the first one again)."""
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,split=2")
    data = [[s.cpu().numpy() for s in _snapshots(dims, nt)] for dims, nt in series]      # (host arrays: every slice owns a field array too)
    (dims0, nt0) = series[0]

    def first_pass(ctx, drop_and_remesh):
        for t in range(nt0):
            ctx.push_scalar_slice(t, data[0][t])
        ctx.invalidate_masks(); ctx.sweep_series_submit(range(nt0), _scopes(gpu, nt0))
        pooled = None
        if drop_and_remesh:
            for t in range(nt0):
                ctx.drop_slice(t)
            _mesh(gpu, ctx, series[1][0], options=False)
            pooled = ctx.array_counts()[1]
        out = _bytes(ctx.sweep_series_complete())
        path = ctx.series_last_path()[0]
        if not drop_and_remesh:
            for t in range(nt0):
                ctx.drop_slice(t)
        return out, path, pooled

    def later(ctx, k):
        dims, nt = series[k]
        _mesh(gpu, ctx, dims)
        for t in range(nt):
            ctx.push_scalar_slice(t, data[k][t])
        out = _bytes(ctx.sweep_series(range(nt), _scopes(gpu, nt)))
        for t in range(nt):
            ctx.drop_slice(t)
        return out

    one = _context(gpu, dims0)
    try:
        got0, path0, pooled = first_pass(one, True)
        got = [got0] + [later(one, k) for k in (1, 2)]
        counts = one.array_counts()
    finally:
        one.close()
    fresh = _context(gpu, dims0)
    try:
        want0, want_path, _ = first_pass(fresh, False)
    finally:
        fresh.close()
    want = [want0]
    for k in (1, 2):
        fresh = _context(gpu, series[k][0])
        try:
            want.append(later(fresh, k))
        finally:
            fresh.close()
    print("paths", path0, want_path, "pooled right after set_mesh", pooled, "counts at the end", counts, "record bytes", [len(b) for b in got], [len(b) for b in want])
    assert path0 == 5 and want_path == 5                      # (a split pass: the drops were parked with it)
    assert pooled == (0, 0, 0)
    assert len(want[0]) > 80 and len(want[1]) > 80            # (there are records to compare)
    assert got[0] == want[0], "the pass that was open across the mesh change"
    assert got[1] == want[1], "the larger lattice afterwards"
    assert got[2] == want[2], "the first lattice again"


def _stream_steps(gpu, ctx, push, nsteps):
    """the tracker's streaming step: push t + 1, prepare (t, t + 1), sweep t, drop t - 1 -> `allocated` after every step"""
    push(0)
    seen = []
    for t in range(nsteps):
        push(t + 1)
        rm = ctx.slices_prepare([t, t + 1])
        factor = gpu.scaling_factor(min(rm[t][0], rm[t + 1][0]))[0]
        ctx.sweep(t, gpu.SCOPE_BOTH, factor)
        if t >= 1:
            ctx.drop_slice(t - 1)
        seen.append(ctx.array_counts()[0])
    return seen


@pytest.mark.parametrize("case", ["scalar 16 x 16", "vector 16 x 16 with V and J", "scalar 9 x 9 x 9"])
def test_streaming_allocates_nothing_once_under_way(gpu, case):
    """Eight streaming steps from host arrays.  Derived from the code: a host array is copied into a field array out of the pool
    (push_common: one per array given -- S; or V and J), and ftkx_slices_prepare gives every slice it sees for the first time a mask
    array and, where the mesh has summarised masks, a summary array (ensure_mask_arrays); the sweep finds them there.  Step t pushes slice
    t + 1 while t - 1, t are resident (3 slices' arrays live, the pool empty until the first drop at the end of step 1) and then drops
    t - 1, whose arrays -- 3 at most per class, below the cap of 12 -- the next push and prepare take out again under the same bytes.
    So from the end of step 1 on: field = 3 x (arrays per slice), mask = 3, summary = 3 or 0; nothing is allocated afterwards, and in
    particular `allocated` after step 3 is `allocated` after step 8."""
    dims = (9, 9, 9) if "9 x 9 x 9" in case else (16, 16)
    vector = case.startswith("vector")
    # smooth data (few cells survive the cull, so that every step is swept the same way); a vector slice: two snapshots as components
    steps = [s.cpu().numpy() for s in _snapshots(dims, 9)]
    ctx = _context(gpu, dims)
    try:
        summarised = 1 if ctx.packed_masks_bytes()[0] else 0
        if vector:
            push = lambda t: ctx.push_slice(t, np.stack([steps[t], steps[(t + 3) % 9]], axis=-1), np.stack([steps[(t + k) % 9] for k in range(4)], axis=-1))
        else:
            push = lambda t: ctx.push_scalar_slice(t, steps[t])
        seen = _stream_steps(gpu, ctx, push, 8)
    finally:
        ctx.close()
    print(case, "allocated (field, mask, summary) after steps 1 .. 8:", seen)
    assert seen[2] == seen[7]
    assert all(a == (3 * (2 if vector else 1), 3, 3 * summarised) for a in seen[1:]), seen


def test_deferred_split_passes_allocate_nothing_once_under_way(gpu, monkeypatch):
    """Batches of three steps under FTKX_SERIES_HOOKS split=2, collected one batch late: batch b pushes slices 3b + 1 .. 3b + 3 (slice 0 with
    batch 0), submits the pass over steps 3b .. 3b + 2 (slices 3b .. 3b + 3, masks invalidated first so that all four are rebuilt), then
    completes pass b - 1 and drops slices 3b - 3 .. 3b - 1.  Derived from the code: the drops happen while pass b, split, is the newest one
    open, so the slices are PARKED with it (free_slice) and reach the pool when pass b completes, in batch b + 1 -- after that batch's
    pushes.  Slice 3b is in pass b - 1 and in pass b, which rebuilds its masks while the tail of b - 1 may read them: it gets other arrays,
    the old pair is RETIRED to pass b - 1 (series_retire_masks) and reaches the pool when b - 1 completes, in batch b.
    Field arrays: batch 0 allocates 4, batches 1 and 2 three each (nothing has come back yet: the first parked slices, of batch 1, come
    back when pass 1 completes at the end of batch 2), batch 3 takes the three that came back: 10, and it stays there.
    Mask arrays (and summary arrays where the mesh has them): pass 0 allocates 4; pass 1 needs 4 with the pool empty: 8; completing pass 0
    brings the retired pair of slice 3 back, so pass 2 allocates 3: 11; completing pass 1 brings back one retired pair and three parked
    slices' -- the four that pass 3 needs: 11 from the third batch on."""
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,split=2")
    dims, nb = (16, 16), 6
    steps = [s.cpu().numpy() for s in _snapshots(dims, 3 * nb + 1)]
    ctx = _context(gpu, dims)
    seen, paths = [], []
    try:
        summarised = 1 if ctx.packed_masks_bytes()[0] else 0
        ctx.push_scalar_slice(0, steps[0])
        for b in range(nb):
            for t in range(3 * b + 1, 3 * b + 4):
                ctx.push_scalar_slice(t, steps[t])
            ctx.invalidate_masks(); ctx.sweep_series_submit(range(3 * b, 3 * b + 3), [gpu.SCOPE_BOTH] * 3)
            if b >= 1:
                ctx.sweep_series_complete()
                paths.append(ctx.series_last_path()[0])
                for t in range(3 * b - 3, 3 * b):
                    ctx.drop_slice(t)
            seen.append(ctx.array_counts()[0])
        ctx.sweep_series_complete()
        paths.append(ctx.series_last_path()[0])
    finally:
        ctx.close()
    print("allocated (field, mask, summary) after batches 1 ..", nb, ":", seen, "paths", paths)
    assert paths == [5] * nb
    assert seen[2] == seen[3] == seen[4] == seen[5]
    assert seen[0] == (4, 4, 4 * summarised) and seen[1] == (7, 8, 8 * summarised) and seen[2] == (10, 11, 11 * summarised), seen


def test_lent_array_is_neither_freed_nor_pooled(gpu):
    """ftkx_push_scalar_slice with on_device = 1, FP64, no smoothing: the caller's device array is adopted as it is.  It is swept, dropped,
    and the context destroyed: the tensor holds the same bytes and is still the caller's to use, no field array was ever allocated, and the
    drop pooled none (the slice's mask array went to the pool, the lent array was let go)."""
    import torch
    dims = (16, 16)
    S = _snapshots(dims, 1)[0]
    before = S.cpu().numpy().tobytes()
    ctx = _context(gpu, dims)
    try:
        ctx.push_scalar_slice(0, S, on_device=1)
        rm = ctx.slices_prepare([0])
        recs = ctx.sweep(0, gpu.SCOPE_ORDINAL, gpu.scaling_factor(rm[0][0])[0])
        resident = ctx.array_counts()
        ctx.drop_slice(0)
        dropped = ctx.array_counts()
    finally:
        ctx.close()
    torch.cuda.synchronize()
    print("records", len(recs), "counts while resident", resident, "after the drop", dropped)
    assert len(recs) > 0
    assert resident[0][0] == 0 and dropped[0][0] == 0 and dropped[1][0] == 0
    assert dropped[0][1] == 1 and dropped[1][1] == 1          # (the mask array was the context's own)
    assert S.cpu().numpy().tobytes() == before
    S.zero_()                                                  # (still allocated, still the caller's)
    torch.cuda.synchronize()
    assert not S.cpu().numpy().any()


def test_temporal_ring_stays_within_k_plus_one_arrays(gpu):
    """K = 5, twelve host snapshots of 16 x 16, every emission dropped before the next push.  The ring holds at most K raw snapshots and one
    more array takes the emission: K + 1 field arrays.  Derived from the code (temporal_push_common, temporal_emit): pushes 1 and 2 allocate
    their ring slots (2); pushes 3, 4, 5 emit while nothing leaves the ring, so each takes a slot AND an array for the emission -- the slot
    comes out of the pool from push 4 on, where the dropped emission before it went: 4, 5, 6; from push 6 on the array that leaves the ring
    takes the emission and the slot is the emission dropped last: 6 for good."""
    K, dims = 5, (16, 16)
    steps = [s.cpu().numpy() for s in _snapshots(dims, 12)]
    ctx = _context(gpu, dims)
    seen, emitted = [], []
    try:
        ctx.set_temporal_smoothing(1.0, K)
        for a in steps:
            t = ctx.temporal_push(a)
            seen.append(ctx.array_counts()[0][0])
            if t >= 0:
                emitted.append(t)
                ctx.drop_slice(t)
    finally:
        ctx.close()
    print("field arrays allocated after pushes 1 .. 12:", seen, "emitted", emitted)
    assert emitted == list(range(10))                          # (pushes 3 .. 12)
    assert max(seen) <= K + 1
    assert seen == [1, 2, 4, 5] + [6] * 8
