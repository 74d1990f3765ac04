"""Meshes whose array lattice does not begin at the origin and whose core lies strictly inside the domain, for
tests/test_gpu_mesh_geometry.py; what each of them has to show is asserted without a GPU in tests/test_mesh_cases.py.

Every kernel that turns a lattice coordinate into an array index subtracts Mesh::ext_st, and every kernel that enumerates corners walks
Mesh::core_st / core_sz: with ext_st = 0 and core = domain -- every other mesh of the suite but one -- a dropped `- m.ext_st[d]` or a
core mistaken for the domain changes nothing.  Here the array begins at ORIGIN = (5, 7[, 3]), no multiple of 4, 8 or 16; the domain is the
usual inset of the array (scalar input: the vertices 2 .. D - 2, vector input: 1 .. D - 2, as the reference's callers set it); the
core is smaller than the domain on every face.  Along x, relative to the array:

  ragged   the core's first column = 3 (mod 8), its last = 4 (mod 8): the first and the last word of 8 mask bytes are partial
  aligned  the core's first column = 0 (mod 8), its last = 7 (mod 8): whole words only

Along y the core is the domain's rows less two below and one above -- its last row is D - 3, where record_is_fast's array condition
(sweep_device.hpp) fails --, along z less one below and two above.  The shapes are the smallest that select each mask kernel family in
plan_masks (mask_plan.hpp); FAMILY names what ftkx_last_mask_kernel() has to say.  Ragged cores carry values on a 1/64 grid (the factor
stays 256, no determinant can overflow, the strict-sign cull is legal at every vertex), aligned cores rough values (the cumulative sum of
normals x 0.125: factors of 2^9 to 2^21, in three of the 3D cases vertices under the per-vertex overflow rule).  One case is `huge`: every
determinant may wrap.

The reference of a case is one_launch_cases.reference: the CPU oracle, swept step by step on the case's own (domain, core, array
lattice) -- the handling of an origin that tests/test_offset_golden.py pins to the real reference."""
import zlib

import numpy as np

from one_launch_cases import BOTH, INTERVAL, ORDINAL, Case, _cache, derived, reference  # noqa: F401  (reference: re-exported)

ORIGIN = {2: [5, 7], 3: [5, 7, 3]}

# shape -> (nv: 1 scalar / nd vector, steps, the kernel plan_masks picks, FTKX_MASK_PLAN, does the mesh carry summaries)
SHAPES = [
    ((40, 21, 11), 1, 3, "ftkx::mask_march6_kernel<2, 4, 4, false>", None, True),
    ((136, 19, 9), 1, 2, "ftkx::mask_march6_kernel<2, 4, 4, false>", None, True),
    ((42, 19, 9), 1, 2, "ftkx::mask_march6_kernel<2, 4, 4, false>", None, False),          # DW even, not a multiple of 8: no summaries
    ((40, 23), 1, 4, "ftkx::mask_march4_kernel<2, false, 1, 8>", None, True),
    ((136, 21), 1, 3, "ftkx::mask_march4_kernel<2, false, 1, 8>", None, True),
    ((40, 37), 1, 3, "ftkx::mask_rows2_kernel<8>", "rows=2", True),
    ((40, 23), 2, 3, "ftkx::mask_vec_kernel<2>", None, True),
    ((24, 13, 9), 3, 3, "ftkx::mask_vec_kernel<3>", None, True),
    ((256, 13), 2, 3, "ftkx::mask_vec2_kernel<2>", None, True),
    ((256, 9, 7), 3, 2, "ftkx::mask_vec2_kernel<3>", None, True),
    ((41, 23), 1, 3, "ftkx::mask_kernel<2>", None, False),
    ((25, 13, 9), 3, 3, "ftkx::mask_kernel<3>", None, False),
]


class MeshCase(Case):
    """a Case of one_launch_cases with what the mesh tests ask of it: placement ("ragged" | "aligned"), kind ("grid64" | "rough" | "huge"),
    family (the mask kernel's name), mask_plan (FTKX_MASK_PLAN or None), summaries (does plan_masks give the mesh summaries)"""


def _rng(name, t):
    return np.random.default_rng([zlib.crc32(name.encode()), int(t)])


def _values(kind, rng, shape, t):
    if kind == "grid64":       # (tests/test_gpu_properties.py: test_mask_kernel_generations_agree)
        return np.round(rng.standard_normal(shape) * 2) * 0.25 + rng.integers(-2, 3, size=shape) / 64.0
    if kind == "rough":        # (tests/test_gpu_fuzz.py: _field)
        return np.cumsum(rng.standard_normal(shape), axis=-1) * 0.125 + 0.05 * t
    if kind == "huge":         # quantised magnitudes that wrap the determinants: one bump of height 7e8 that moves
        grids = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing="ij")
        r2 = sum((g - (0.1 + 0.05 * t)) ** 2 for g in grids)
        return np.exp(-3.0 * r2) * 7e8
    raise ValueError(kind)


def field(name, dims, nv, kind):
    """t -> the array of timestep t (scalar: shape reversed dims; vector: (..., nd)); the same values whenever it is asked"""
    shape = tuple(reversed(dims))

    def f(t):
        rng = _rng(name, t)
        if nv == 1:
            return _values(kind, rng, shape, t)
        return np.stack([_values(kind, rng, shape, t) for _ in range(nv)], axis=-1)
    return f


def x_core(placement, lo, hi):
    """(first, last) column of the core relative to the array, strictly inside the domain's columns lo .. hi"""
    if placement == "ragged":
        first, last = 3, (hi - 1 - 4) // 8 * 8 + 4
    else:
        first, last = 8, (hi - 1 - 7) // 8 * 8 + 7
    assert lo < first < last < hi, (placement, lo, hi, first, last)
    return first, last


def make(name, dims, nv, nt, placement, kind, family, mask_plan=None, summaries=False, origin=None):
    nd = len(dims)
    org = list(ORIGIN[nd] if origin is None else origin)
    lo = 2 if nv == 1 else 1
    rel = [(lo, d - 2) for d in dims]                         # the domain's vertices relative to the array, per axis, inclusive
    box = [x_core(placement, *rel[0]), (rel[1][0] + 2, rel[1][1] - 1)] + ([(rel[2][0] + 1, rel[2][1] - 2)] if nd == 3 else [])
    dom = ([o + r[0] for o, r in zip(org, rel)], [r[1] - r[0] + 1 for r in rel])
    core = ([o + b[0] for o, b in zip(org, box)], [b[1] - b[0] + 1 for b in box])
    c = MeshCase(name, dims, range(nt), field(name.split("@")[0], dims, nv, kind), scopes=[BOTH] * (nt - 1) + [ORDINAL], nv=nv, dom=dom, core=core, ext_st=org)
    c.placement, c.kind, c.family, c.mask_plan, c.summaries, c.origin = placement, kind, family, mask_plan, summaries, org
    return c


def at_origin_zero(c):
    """the same arrays, the same domain and core relative to them, the array lattice at 0"""
    z = make(c.name + "@0", c.dims, c.nv, c.n, c.placement, c.kind, c.family, c.mask_plan, c.summaries, origin=[0] * c.nd)
    assert all(np.array_equal(z.slices()[t], c.slices()[t]) for t in c.slice_ts)
    return z


def whole_domain(c):
    """the same mesh with core = domain"""
    w = make(c.name, c.dims, c.nv, c.n, c.placement, c.kind, c.family, c.mask_plan, c.summaries)
    w.name, w.core = c.name + "@whole", w.dom
    return w


def _label(dims, nv):
    return f"{len(dims)}d_{'scalar' if nv == 1 else 'vector'}_" + "x".join(str(d) for d in dims)


def _make_cases():
    out = []
    for dims, nv, nt, family, plan, summaries in SHAPES:
        for placement, kind in (("ragged", "grid64"), ("aligned", "rough")):
            out.append(make(f"{_label(dims, nv)}_{placement}", dims, nv, nt, placement, kind, family, plan, summaries))
    out.append(make("3d_scalar_40x21x11_huge", (40, 21, 11), 1, 3, "ragged", "huge", SHAPES[0][3], None, True))
    return {c.name: c for c in out}


def cases():
    if "mesh_cases" not in _cache:
        _cache["mesh_cases"] = _make_cases()
    return _cache["mesh_cases"]


def planned(c, u_rows=None, rows=False):
    """(the kernel's name, has_summary) plan_masks gives the case's shape under its FTKX_MASK_PLAN and FTKX_U_ROWS = u_rows, through
    tests/hostcheck/hostcheck.cpp as tests/test_mask_plan.py drives it; rows=True: (name, has_summary, the rows a summary byte stands for)"""
    import ctypes as C
    import os
    import subprocess
    import tempfile
    if "plan_lib" not in _cache:
        so = os.path.join(tempfile.mkdtemp(prefix="mesh_plan_"), "libhostcheck_plan.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "hostcheck.cpp")])
        L = C.CDLL(so)
        L.hc_mask_plan.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_char_p]
        L.hc_mask_plan.restype = None
        _cache["plan_lib"] = L
    d = list(c.dims) + [1] * (3 - c.nd)
    shape = (C.c_int * 6)(c.nd, int(c.nv == 1), d[0], d[1], d[2], (d[0] + 7) // 8 * 8 + 8)
    out = (C.c_longlong * (14 + 2 * 47))()
    name = C.create_string_buffer(64)
    _cache["plan_lib"].hc_mask_plan(shape, c.mask_plan.encode() if c.mask_plan else None, None if u_rows is None else str(u_rows).encode(), c.n + 1, 0, out, name)
    return (name.value.decode(), bool(out[2]), int(out[3])) if rows else (name.value.decode(), bool(out[2]))


def array_rel(c, recs):
    """the records' corners relative to the array lattice, one column per axis"""
    return recs["corner"][:, :c.nd].astype(np.int64) - np.array(c.ext[0])


def is_fast_box(c, recs):
    """record_is_fast's array condition (sweep_device.hpp): corner - 2 .. corner + 3 inside the array, on every axis"""
    a = array_rel(c, recs)
    return np.all((a >= 2) & (a + 3 < np.array(c.dims)), axis=1)


def cull_counts(c):
    """(cells, removable): the (step, corner) pairs of the case, and those the strict-sign cull may drop -- every scope the step asks for
    has a component whose quantised value trunc(v * factor) is strictly positive, or strictly negative, at all 2^nd vertices of the cell
    (interval: in both slices); a vertex outside the domain, or one with a quantised component of safe_m and more, carries no sign
    (mask_kernels.hip, cull_exact_kernels.hip, classify_value in sweep_device.hpp).  From the oracle's
    gradients and factors alone"""
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
        big = (np.abs(q) >= (727041 if c.nd == 3 else 1239850262)).any(-1)      # kSafeM3 / kSafeM2 (sweep_params.hpp): a determinant with it may wrap
        bits = np.concatenate([q > 0, q < 0], axis=-1) & (inside & ~big)[..., None]
        out = None
        for o in range(2 ** c.nd):
            idx = tuple(slice(box[d][0] + ((o >> d) & 1), box[d][1] + ((o >> d) & 1) + 1) for d in reversed(range(c.nd)))
            out = bits[idx] if out is None else out & bits[idx]
        return out
    cells = removable = 0
    for t, scope, factor in zip(c.ts, c.scopes, factors):
        cur = cube(t, factor)
        gone = (cur & cube(t + 1, factor)).any(-1) if scope & INTERVAL else cur.any(-1)
        cells += gone.size; removable += int(gone.sum())
    return cells, removable


def aux_field(c, t, which):
    """a field foreign to the case, of the extent of its arrays: uniform in +-10^3, the same values whenever it is asked"""
    return np.random.default_rng([zlib.crc32(c.name.encode()), int(t), 77 + int(which)]).uniform(-1e3, 1e3, size=tuple(reversed(c.dims)))


def aux_expected(c, which):
    """scalar[1 + which] of every record of reference(c), in its order: what the oracle lerps when aux_field(c, t, which) stands in for S,
    the vector field, the Jacobian and the factors being the case's own"""
    import pyoracle as O
    key = ("aux", c.name, which)
    if key not in _cache:
        r, factors, _ = reference(c)
        f = {t: derived(c, a) for t, a in c.slices().items()}
        B = {t: aux_field(c, t, which) for t in c.slice_ts}
        tags, vals = [], []
        for t, scope, factor in zip(c.ts, c.scopes, factors):
            for sc in (ORDINAL, INTERVAL):
                if not scope & sc:
                    continue
                u = t + 1 if sc == INTERVAL else t
                nxt = sc == INTERVAL
                got = O.sweep(c.nd, sc, t, c.dom, c.core, c.ext, (f[t][0], f[u][0] if nxt else None), (f[t][1], f[u][1] if nxt else None), (B[t], B[u] if nxt else None), factor,
                              jacobian_symmetric=(c.nv == 1), tag_mode=c.tag_mode, nthreads=4)
                tags.append(got["tag"]); vals.append(got["scalar"][:, 0])
        tags, vals = np.concatenate(tags), np.concatenate(vals)
        order = np.argsort(tags, kind="stable")
        assert np.array_equal(tags[order], r["tag"]) and len(np.unique(tags)) == len(tags)
        out = vals[order]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def reference_rectilinear(c, rect):
    """the records of reference(c) with REGULAR_COORDS_RECTILINEAR coordinates: rect[d] is read at the vertex's lattice coordinate"""
    import pyoracle as O
    _, factors, _ = reference(c)
    f = {t: derived(c, a) for t, a in c.slices().items()}
    recs = []
    for t, scope, factor in zip(c.ts, c.scopes, factors):
        for sc in (ORDINAL, INTERVAL):
            if not scope & sc:
                continue
            nxt = f[t + 1] if sc == INTERVAL else (None, None, None)
            recs.append(O.sweep(c.nd, sc, t, c.dom, c.core, c.ext, (f[t][0], nxt[0]), (f[t][1], nxt[1]), (f[t][2], nxt[2]) if c.nv == 1 else None, factor,
                                jacobian_symmetric=(c.nv == 1), tag_mode=c.tag_mode, nthreads=4, rectilinear=rect))
    r = np.concatenate(recs)
    return r[np.argsort(r["tag"], kind="stable")]


def masks_need_the_vertex_rule(c):
    """does a step of the case read a slice whose largest |v|, quantised under the step's factor, could take a determinant out of int64
    (batch_plan.hpp: overflow_free -- M = floor(max |v| x factor) + 1, 24 M^3 (3D) or 6 M^2 (2D) below 2^63)?  The device-driven series
    pass builds its masks without the per-vertex rule: it then declines with SERIES_MASKS_INVALID and the host-driven batch sweeps the steps"""
    _, factors, _ = reference(c)
    top = {t: float(np.abs(derived(c, a)[0]).max()) for t, a in c.slices().items()}
    for t, scope, factor in zip(c.ts, c.scopes, factors):
        for u in (t, t + 1) if scope & INTERVAL else (t,):
            m = int(np.floor(top[u] * float(factor))) + 1
            if not (24 * m ** 3 < 2 ** 63 if c.nd == 3 else 6 * m ** 2 < 2 ** 63):
                return True
    return False
