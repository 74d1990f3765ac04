"""The context's buffers (ftk_amd/csrc/ctx_block.hpp) on the device: every one is admitted by its own bytes, so a context serves calls whose
buffers grow, shrink and change their element size in any order exactly as a fresh context serves each of them."""
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
