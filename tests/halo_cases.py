"""What links two ranks of a series cut into timestep slabs, on the meshes of tests/mesh_cases.py (array lattice at (5, 7[, 3]), core strictly
inside the domain), for tests/test_gpu_halo_geometry.py; what each premise has to show is asserted without a GPU in tests/test_halo_cases.py.

The kernels of the slab pass (dist_kernels.hip) and of the compact halo (halo_kernels.hip) turn core-linear cell indices into array
addresses (core_st + c - ext_st, clamped to ext_sz), summary-byte positions into mask-word indices (row * P / 8 + g; urow / urows; u_rows of
1, 4 or 16) and write rows clipped at the last partial block of DH: with ext_st = 0 and core = domain a wrong origin or a wrong core
cannot show.  Here are, from the oracle and the mask plan alone: the cuts, the bounds a request's cell count has to keep, the cells it
must contain, which slabs the device-driven pass has to decline, and plain numpy references of the word compaction and the patch
addresses.

A cut is a tuple of slab bounds (0, b1, .., nt): slab r owns the slices b[r] .. b[r + 1] - 1.  Every cut into two slabs is taken, one per
interior slice boundary -- tslab.slab_range yields only the even one of them; where a cut IS the even partition (every two-slab cut at
nt // 2, every cut into one step per rank) test_halo_cases.py holds slab_range / owner_of here to tslab's."""
import numpy as np

import mesh_cases as M
from mesh_cases import INTERVAL, derived, reference

# the boundaries the limit tests use: (case, cut, the lower slab's last step t).  Neither rank of them declines, L_t >= 65 (a request
# crosses a wavefront); one 2D, one 3D.  tests/test_halo_cases.py holds them to that.
LIMIT_CASES = [("2d_scalar_40x23_ragged", (0, 2, 4), 1), ("3d_scalar_40x21x11_ragged", (0, 2, 3), 1)]


def cuts(c):
    """every cut of the case into two slabs, and for three steps and more the cut into one step per rank (a middle rank has both neighbours)"""
    nt = c.n
    out = [(0, b, nt) for b in range(1, nt)]
    if nt >= 3:
        out.append(tuple(range(nt + 1)))
    return out


def slab_range(cut, rank):
    return cut[rank], cut[rank + 1]


def owner_of(cut, t):
    for r in range(len(cut) - 1):
        if cut[r] <= t < cut[r + 1]:
            return r
    raise ValueError(t)


def boundaries(cut):
    """(lower rank, t): the lower slab's last step t, whose interval sweep reads the slice t + 1 of the next rank"""
    return [(r, cut[r + 1] - 1) for r in range(len(cut) - 2)]


def cull_counts_per_step(c):
    """mesh_cases.cull_counts per step and scope: [{scope: (cells_t, removable_t)}], ORDINAL and INTERVAL apart -- the strict-sign rule
    applied to the scope's own slices (interval: both).  Their sum over the scopes a step asks for is NOT cull_counts' (a BOTH step counts a
    cell once there, removable when every scope lets it go: the interval's condition)"""
    _, factors, _ = reference(c)
    rel_lo = [c.dom[0][d] - c.ext[0][d] for d in range(c.nd)]
    rel_hi = [rel_lo[d] + c.dom[1][d] - 1 for d in range(c.nd)]
    box = [(c.core[0][d] - c.ext[0][d], c.core[0][d] - c.ext[0][d] + c.core[1][d] - 1) for d in range(c.nd)]
    inside = np.ones(tuple(reversed(c.dims)), dtype=bool)
    for d in range(c.nd):
        i = np.arange(c.dims[d])
        shape = [1] * c.nd; shape[c.nd - 1 - d] = c.dims[d]
        inside &= ((i >= rel_lo[d]) & (i <= rel_hi[d])).reshape(shape)

    def cube(t, factor):
        q = np.trunc(derived(c, c.slices()[t])[0] * float(factor))
        big = (np.abs(q) >= (727041 if c.nd == 3 else 1239850262)).any(-1)      # kSafeM3 / kSafeM2 (sweep_params.hpp)
        bits = np.concatenate([q > 0, q < 0], axis=-1) & (inside & ~big)[..., None]
        out = None
        for o in range(2 ** c.nd):
            idx = tuple(slice(box[d][0] + ((o >> d) & 1), box[d][1] + ((o >> d) & 1) + 1) for d in reversed(range(c.nd)))
            out = bits[idx] if out is None else out & bits[idx]
        return out
    out = []
    for t, scope, factor in zip(c.ts, c.scopes, factors):
        cur = cube(t, factor)
        per = {M.ORDINAL: (int(cur.any(-1).size), int(cur.any(-1).sum()))}
        if scope & INTERVAL:
            both = (cur & cube(t + 1, factor)).any(-1)
            per[INTERVAL] = (int(both.size), int(both.sum()))
        out.append(per)
    return out


def request_bounds(c, t):
    """(L_t, C_t, R_t) of the boundary step t: a request for the slice t + 1 holds at least L_t = cells_t - removable_t cells (the cull may
    not drop more), at most C_t = cells_t, and every cell of R_t -- the corners of the reference's interval records at t, core-linear (x fastest)"""
    key = ("halo_bounds", c.name, t)
    if key not in M._cache:
        cells, removable = cull_counts_per_step(c)[c.ts.index(t)][INTERVAL]
        r, _, _ = reference(c)
        at = r[(r["timestep"] == t) & (r["ordinal"] == 0)]
        lin = np.zeros(len(at), dtype=np.int64)
        for d in reversed(range(c.nd)):
            lin = lin * c.core[1][d] + (at["corner"][:, d] - c.core[0][d])
        R = np.unique(lin)
        R.setflags(write=False)
        M._cache[key] = (cells - removable, cells, R)
    return M._cache[key]


def slab_needs_the_vertex_rule(c, cut, rank):
    """mesh_cases.masks_need_the_vertex_rule for the steps of ONE slab: does a step of this rank read a slice (its own, or the halo behind its
    last step) whose largest |v| under the step's factor could take a determinant out of int64?"""
    _, factors, _ = reference(c)
    t0, t1 = slab_range(cut, rank)
    top = {t: float(np.abs(derived(c, a)[0]).max()) for t, a in c.slices().items()}
    for t, scope, factor in zip(c.ts, c.scopes, factors):
        if not t0 <= t < t1:
            continue
        for u in (t, t + 1) if scope & INTERVAL else (t,):
            m = int(np.floor(top[u] * float(factor))) + 1
            if not (24 * m ** 3 < 2 ** 63 if c.nd == 3 else 6 * m ** 2 < 2 ** 63):
                return True
    return False


def must_decline(c, cut, rank):
    """the device-driven pass of this slab has to decline (SERIES_MASKS_INVALID; a rank with a halo asks -1)"""
    return c.kind == "huge" or slab_needs_the_vertex_rule(c, cut, rank)


def summary_layout(dims, u_rows):
    """(ngroups, UP, P, urows, DH, DD) of a summary array: ceil(DW / 8) groups of 8 mask bytes per row, rows of UP summary bytes, mask rows of P
    bytes, ceil(DH / u_rows) summary rows per plane"""
    DW, DH, DD = dims[0], dims[1], (dims[2] if len(dims) == 3 else 1)
    ngroups = (DW + 7) // 8
    return ngroups, (ngroups + 7) // 8 * 8 + 8, (DW + 7) // 8 * 8 + 8, (DH + u_rows - 1) // u_rows, DH, DD


def compacted(U, dims, u_rows):
    """the sorted indices of the 8-byte mask words a summary array implies: for every byte of U at (plane k, block row yb, group g < ngroups)
    that is 0, the words ((k * DH + y) * P) // 8 + g of the rows y = yb * u_rows .. min(DH, (yb + 1) * u_rows) - 1.  Bytes at g >= ngroups
    are padding.  Plain loops: the reference of compact_words_kernel and dist_export_kernel"""
    ngroups, UP, P, urows, DH, DD = summary_layout(dims, u_rows)
    U = np.asarray(U, dtype=np.uint8).reshape(-1)
    assert U.size >= UP * urows * DD, (U.size, UP, urows, DD)
    out = []
    for k in range(DD):
        for yb in range(urows):
            row = U[(k * urows + yb) * UP:(k * urows + yb) * UP + ngroups]
            for g in np.flatnonzero(row == 0):
                for y in range(yb * u_rows, min(DH, (yb + 1) * u_rows)):
                    out.append(((k * DH + y) * P) // 8 + int(g))
    return np.array(sorted(out), dtype=np.int64)


def patch_addresses(c, cells):
    """per core-linear cell index, the flat array index (x fastest) of every element of its patch: corner - ext_st - 2 .. + 3 on every axis,
    clamped to the array -> (len(cells), 6 ** nd)"""
    nd, dims = c.nd, c.dims
    lin = np.asarray(cells, dtype=np.int64)
    q = np.arange(6 ** nd)
    at = np.zeros((len(lin), 6 ** nd), dtype=np.int64)
    stride = 1
    for d in range(nd):
        corner = c.core[0][d] + lin % c.core[1][d] - c.ext[0][d]; lin = lin // c.core[1][d]
        x = np.clip(corner[:, None] - 2 + (q % 6)[None, :], 0, dims[d] - 1); q = q // 6
        at += x * stride; stride *= dims[d]
    return at
