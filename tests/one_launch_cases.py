"""Series that sit ON the limits of the one-launch pass (ftk_amd/csrc/one_kernel.hip), for tests/test_gpu_one_launch.py; what each of
them has to show is asserted without a GPU in tests/test_one_launch_cases.py.

The pass is one persistent launch: the (step, corner) range cs = step * cells + corner index is cut into blocks of BS = 128 (2D) or 64 (3D)
consecutive cs, nblocks = ceil(cells * n / BS); nwg = max(8, min(256, (nblocks + 3) // 4)) workgroups take bpw = ceil(nblocks / nwg)
consecutive blocks each and park the order keys of the simplices that passed in LDS, kOneKeys at most.  plan() asks
ftk_amd/csrc/one_plan.hpp -- the functions series.hip calls -- for eligibility, nblocks and nwg through tests/hostcheck/one_plan.cpp, and
limits() reads the kOne* constants of ftk_amd/csrc/sweep_params.hpp from the same program: nothing of them is retyped here.

The reference of a case is the CPU oracle (oracle/pyoracle.py) driven step by step the way its own track() drives it -- the sticky minimum
of the slices' resolutions over the WHOLE array, the factor from it, ftko_sweep per scope -- on the case's own mesh, steps and scopes,
stably sorted by tag under TAG_EXACT64.  parked() counts the keys each workgroup parks from the records' corner and timestep.

A mesh is (starts, sizes) per axis as ftkx_set_mesh takes it.  Unless a case says otherwise: scalar input, array start 0, domain = core =
the vertices 2 .. D - 3 of every axis, every step BOTH."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORDINAL, INTERVAL, BOTH = 1, 2, 3

_cache = {}


def _program():
    if "exe" not in _cache:
        d = tempfile.mkdtemp(prefix="one_plan_")
        exe = os.path.join(d, "one_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(HERE, "hostcheck", "one_plan.cpp")])
        _cache["exe"] = exe
    return _cache["exe"]


def _ask(lines):
    out = subprocess.run([_program()], input="".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()
    return out[0], out[1:]


def limits():
    """the kOne* constants, the block sizes and the status bits as the product's headers have them"""
    if "limits" not in _cache:
        head, _ = _ask([])
        _cache["limits"] = {k: int(v) for k, v in (w.split("=") for w in head.split())}
    return _cache["limits"]


def plan_of(nd, n, k, cells, n_vertices, last_hits=0):
    """-> dict(eligible, nblocks, nwg, bpw, bs) from one_plan.hpp"""
    _, rows = _ask([f"{nd} {n} {k} {cells} {n_vertices} {last_hits}\n"])
    e, nblocks, nwg = (int(v) for v in rows[0].split())
    return dict(eligible=bool(e), nblocks=nblocks, nwg=nwg, bpw=-(-nblocks // nwg), bs=limits()["block2" if nd == 2 else "block3"])


class Case:
    def __init__(self, name, dims, ts, fields, *, scopes=None, nv=1, dom=None, core=None, ext_st=None, tag_mode=2, degrees=False, bounds=None,
                 given_j=False, expect="taken"):
        self.name, self.dims, self.nd, self.nv = name, tuple(dims), len(dims), nv
        self.ts = [int(t) for t in ts]
        self.scopes = [BOTH] * len(self.ts) if scopes is None else list(scopes)
        self.fields = fields                                    # t -> array (scalar: shape reversed dims; vector: (..., nd))
        self.ext = (list(ext_st) if ext_st else [0] * self.nd, list(self.dims))
        lo = 2 if nv == 1 else 1
        self.dom = dom if dom is not None else ([e + lo for e in self.ext[0]], [d - 2 * lo for d in self.dims])
        self.core = core if core is not None else self.dom
        self.tag_mode, self.degrees, self.bounds, self.given_j = tag_mode, degrees, bounds, given_j
        self.expect = expect                                    # "taken" | "not" (another path, no decline) | status bit of the decline

    @property
    def n(self):
        return len(self.ts)

    @property
    def slice_ts(self):
        """the slices the steps read, in time order (series.hip: series_steps)"""
        out = []
        for t, s in zip(self.ts, self.scopes):
            if not out or out[-1] != t:
                out.append(t)
            if s & INTERVAL:
                out.append(t + 1)
        return out

    @property
    def cells(self):
        return int(np.prod(self.core[1], dtype=np.int64))

    @property
    def n_vertices(self):
        return int(np.prod(self.dims, dtype=np.int64))

    def plan(self, last_hits=0):
        return plan_of(self.nd, self.n, len(self.slice_ts), self.cells, self.n_vertices, last_hits)

    def slices(self):
        """t -> array, made once, never changed"""
        key = ("slices", self.name)
        if key not in _cache:
            d = {t: np.ascontiguousarray(self.fields(t), dtype=np.float64) for t in self.slice_ts}
            for a in d.values():
                a.setflags(write=False)
            _cache[key] = d
        return _cache[key]


def derived(case, a):
    """(V, J, S) of one snapshot as the reference's tracker derives them (ftko_track)"""
    import pyoracle as O
    if case.nv == 1:
        V = O.gradient2D(a) if case.nd == 2 else O.gradient3D(a)
        J = O.jacobian2D(V, True) if case.nd == 2 else O.jacobian3D(V)
        return V, J, a
    J = O.jacobian2D(a, False) if case.nd == 2 else O.jacobian3D(a)
    return a, J, None


def reference(case, running=None):
    """-> (records stably sorted by tag, factors per step, the slices' resolutions in slice order); once per case"""
    import pyoracle as O
    key = ("ref", case.name, running)
    if key in _cache:
        return _cache[key]
    sl = case.slices()
    f = {t: derived(case, a) for t, a in sl.items()}
    res = {t: O.resolution(f[t][0]) for t in sl}
    run = np.finfo(np.float64).max if running is None else running
    sts, j, recs, factors = case.slice_ts, 0, [], []
    for t, scope in zip(case.ts, case.scopes):
        while j < len(sts) and sts[j] <= t + 1:
            run = min(run, res[sts[j]]); j += 1
        factor = O.scaling_factor(run)[0]
        factors.append(int(factor))
        for sc in (ORDINAL, INTERVAL):
            if not scope & sc:
                continue
            nxt = f[t + 1] if sc == INTERVAL else (None, None, None)
            S = (f[t][2], nxt[2]) if case.nv == 1 else None
            recs.append(O.sweep(case.nd, sc, t, case.dom, case.core, case.ext, (f[t][0], nxt[0]), (f[t][1], nxt[1]), S, factor,
                                jacobian_symmetric=(case.nv == 1), compute_degrees=case.degrees, tag_mode=case.tag_mode, nthreads=min(8, os.cpu_count() or 1),
                                bounds=case.bounds))
    r = np.concatenate(recs) if recs else np.zeros(0, dtype=O.REC_DTYPE)
    r = r[np.argsort(r["tag"], kind="stable")]
    r.setflags(write=False)
    _cache[key] = (r, factors, [res[t] for t in sts])
    return _cache[key]


def parked(case):
    """keys per workgroup of the launch, from the reference's records: cs = step * cells + corner index, workgroup = cs // BS // bpw"""
    r, _, _ = reference(case)
    p = case.plan()
    step = np.searchsorted(np.array(case.ts), r["timestep"])
    lin = np.zeros(len(r), dtype=np.int64)
    for d in reversed(range(case.nd)):
        lin = lin * case.core[1][d] + (r["corner"][:, d] - case.core[0][d])
    cs = step.astype(np.int64) * case.cells + lin
    return np.bincount(cs // p["bs"] // p["bpw"], minlength=p["nwg"]), np.bincount(cs // p["bs"], minlength=p["nblocks"])


# ---- fields --------------------------------------------------------------------------------------------------------------------------------

def _grid(dims):
    """coordinate arrays x, y[, z] of shape reversed(dims)"""
    g = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in reversed(dims)], indexing="ij")
    return list(reversed(g))


def moving_extremum(dims, x0, v):
    """sum of (x_d - x0_d - v_d t)^2: one minimum that moves; dyadic parameters keep every factor at 256"""
    g = _grid(dims)
    return lambda t: sum((g[d] - (x0[d] + v[d] * t)) ** 2 for d in range(len(dims)))


def bumps(dims, a, amp=40.0, half=2.0):
    g = _grid(dims)
    out = amp * np.ones(tuple(reversed(dims)))
    for d in range(len(dims)):
        out = out * np.cos(np.pi * (g[d] - a[d]) / half)
    return out


def key_store_field(a, b, q, extra=None):
    """132 x 132: the ramp 3x + 2y; at t = 5 the array rows 42 .. 47 wholly and row 48 up to column q are 40 cos(pi (x - a) / 2) cos(pi (y - b) / 2);
    extra = (row, column, height): one more isolated bump"""
    x, y = _grid((132, 132))
    ramp = 3 * x + 2 * y
    bump = bumps((132, 132), (a, b))

    def f(t):
        s = ramp.copy()
        if t == 5:
            s[42:48, :] = bump[42:48, :]
            s[48, :q + 1] = bump[48, :q + 1]
            if extra:
                s[extra[0], extra[1]] += extra[2]
        return s
    return f


def vertex_rule_field(t):
    """2048 x 1024, zero but for: bumps over the core (vertices 1000 .. 1063 x 500 .. 563) and a margin of 4, whose gradients are all above
    1; the vertex (40, 30) at 2^-22: gradients (gradient2D: differences times D - 1) of 2047 x 2^-22 and 1023 x 2^-22 next to it,
    the smallest non-zero |gradient| of the array -> 13 bits, factor 8192, where the core alone gives 256; the vertex (2000, 1000) at 16:
    the largest |v| (times the factor still far below where a determinant could overflow)"""
    s = np.zeros((1024, 2048))
    b = bumps((2048, 1024), (0.37 + 0.03 * t, 0.61), amp=4.0)
    s[496:568, 996:1068] = b[496:568, 996:1068]
    s[30, 40] = 2.0 ** -22
    s[1000, 2000] = 16.0
    return s


def zigzag(z):
    """g with g(z + 1) - g(z - 1) = (-1)^z: the z-component of the gradient (gradient3D: that difference times D - 1) changes sign from
    every vertex to the next, and its own central difference, the Jacobian's zz entry, is exactly zero at every vertex: a class that
    hangs on the last bits of the cubic's solution (cp_device.hpp: classify3, `fragile`)"""
    return (z // 2) * np.where(z % 2 == 1, 1.0, -1.0)


def plateau(dims, t, edge):
    """zero up to the last axis' coordinate `edge`: gradients exactly zero below it, in every slice.  From edge + 1 on a bowl, 1 + the
    squared distance from a minimum that moves along the first axis.  2D: the minimum lies three and a half vertices behind the edge.
    3D: the bowl is one in x and y, plus zigzag(z): a critical point per cell in z, an eigenvalue of exactly zero in its Jacobian"""
    g = _grid(dims)
    x0 = [d / 2 - 0.75 for d in dims]
    x0[0] += 0.125 * t
    x0[-1] = edge + 3.625
    bowl = 1.0 + sum((g[d] - x0[d]) ** 2 for d in range(2 if len(dims) == 3 else len(dims)))
    if len(dims) == 3:
        bowl = bowl + zigzag(g[2])
    return np.clip(g[-1] - edge, 0.0, 1.0) * bowl


def ambiguous_field(dims):
    """a vector field of 1s whose one other component is v with 1 / v = 2^10 (1 + 2^-40): log2 is 10 + 1.3e-12, nbits hangs on its last bits"""
    v = 1.0 / (2.0 ** 10 * (1.0 + 2.0 ** -40))
    g = _grid(dims)

    def f(t):
        a = np.ones(tuple(reversed(dims)) + (len(dims),))
        a[..., 0] = g[0] - (5.25 + 0.125 * t)
        a[..., 1] = g[1] - (6.5 + 0.25 * t)
        a[1, 1, 0] = v
        return a
    return f, v


def rotation(dims, c, w):
    """a vector field with one centre that moves: (-(y - cy), x - cx) + w * (x - cx, y - cy)"""
    g = _grid(dims)

    def f(t):
        a = np.zeros(tuple(reversed(dims)) + (2,))
        dx, dy = g[0] - (c[0] + 0.125 * t), g[1] - (c[1] + 0.25 * t)
        a[..., 0] = -dy + w * dx
        a[..., 1] = dx + w * dy
        return a
    return f


def with_inf(f, at_t, where):
    def g(t):
        a = f(t).copy()
        if t == at_t:
            a[where] = np.inf
        return a
    return g


def with_value(f, where, v):
    def g(t):
        a = f(t).copy()
        a[where] = v
        return a
    return g


KEYS_OVER = 1     # the over-the-limit case parks kOneKeys + KEYS_OVER keys in its fullest workgroup


def _make_cases():
    L = limits()
    c = []
    # ---- a workgroup's key store exactly full / one over
    c.append(Case("keys_full", (132, 132), range(16), key_store_field(*KEYS_FULL_KNOBS), scopes=[BOTH] * 15 + [ORDINAL]))
    c.append(Case("keys_over", (132, 132), range(16), key_store_field(*KEYS_OVER_KNOBS[:3], extra=KEYS_OVER_KNOBS[3]), scopes=[BOTH] * 15 + [ORDINAL], expect=L["SERIES_OVERFLOW"]))
    # ---- kOneMaxBlocks
    c.append(Case("blocks_2d_at", (260, 132), range(32), moving_extremum((260, 132), (100.25, 60.5), (0.5, 0.25))))
    c.append(Case("blocks_2d_over", (294, 117), range(32), moving_extremum((294, 117), (100.25, 60.5), (0.5, 0.25)), expect="not"))
    c.append(Case("blocks_3d_at", (68, 68, 36), range(4), moving_extremum((68, 68, 36), (30.25, 31.5, 15.125), (0.5, 0.25, 0.125))))
    c.append(Case("blocks_3d_over", (117, 44, 33), range(4), moving_extremum((117, 44, 33), (30.25, 21.5, 15.125), (0.5, 0.25, 0.125)), expect="not"))
    # ---- kOneMaxSteps, kOneMaxSlices
    small = moving_extremum((24, 20), (5.25, 6.5), (0.25, 0.125))
    c.append(Case("steps_47", (24, 20), range(47), small))
    c.append(Case("steps_48", (24, 20), range(48), small, scopes=[BOTH] * 47 + [ORDINAL], expect="not"))
    c.append(Case("gapped_24", (24, 20), range(0, 48, 2), lambda t: small(t / 2.0)))
    c.append(Case("gapped_25", (24, 20), range(0, 50, 2), lambda t: small(t / 2.0), expect="not"))
    # ---- the 2^22-vertex rule
    inner = ([1000, 500], [64, 64])
    c.append(Case("vertices_at", (2048, 1024), [0], vertex_rule_field, core=inner))
    c.append(Case("vertices_over", (2048, 1024), [0, 1], vertex_rule_field, core=inner, expect="not"))
    # ---- blocks that straddle steps, empty blocks, a short last block
    c.append(Case("straddle_2d", (13, 11), range(10), moving_extremum((13, 11), (3.25, 4.5), (0.5, 0.25))))
    c.append(Case("straddle_3d", (7, 7, 7), range(9), moving_extremum((7, 7, 7), (2.75, 3.5, 3.25), (0.125, 0.0625, 0.03125))))
    c.append(Case("no_record", (13, 11), range(10), lambda t: 3 * _grid((13, 11))[0] + 2 * _grid((13, 11))[1] + t))
    c.append(Case("one_record", (13, 11), [0], moving_extremum((13, 11), (6.25, 5.375), (0.0, 0.0)), scopes=[ORDINAL]))
    # ---- the degenerate list exactly full
    c.append(Case("plateau_2d", (40, 16), range(2), lambda t: plateau((40, 16), t, 7.0), scopes=[BOTH, ORDINAL]))
    c.append(Case("plateau_3d", (24, 8, 16), range(2), lambda t: plateau((24, 8, 16), t, 9.0), scopes=[BOTH, ORDINAL]))
    # ---- the fragile list (4 096 records of a fresh context) too small: bumps in x and y plus zigzag(z): a critical point in every cell above and below each of theirs, an eigenvalue of exactly zero in every Jacobian
    c.append(Case("fragile_over", (36, 36, 36), range(2), lambda t: bumps((36, 36), (0.37 + 0.0625 * t, 0.61), half=4.0)[None, :, :] + zigzag(_grid((36, 36, 36))[2]), expect=L["SERIES_OVERFLOW"]))
    # ---- scopes
    c.append(Case("ordinal_only", (24, 20), range(6), small, scopes=[ORDINAL] * 6))
    c.append(Case("interval_only", (24, 20), range(6), small, scopes=[INTERVAL] * 6))
    c.append(Case("mixed_scopes", (24, 20), range(6), small, scopes=[INTERVAL, ORDINAL, BOTH, ORDINAL, INTERVAL, BOTH]))
    # ---- other ways in
    c.append(Case("image_bounds", (24, 20), range(6), small, bounds=[-1.0, 1.0, 0.0, 3.0]))
    c.append(Case("reference_tags", (24, 20), range(6), small, tag_mode=1))
    c.append(Case("work_index_tags", (24, 20), [3], small, scopes=[INTERVAL], tag_mode=0))
    c.append(Case("degrees_2d", (24, 20), range(6), small, degrees=True))
    rot = rotation((24, 20), (7.25, 8.5), 0.25)
    c.append(Case("vector_derived_j", (24, 20), range(6), rot, nv=2))
    c.append(Case("vector_given_j", (24, 20), range(6), rot, nv=2, given_j=True))
    c.append(Case("offset_mesh", (24, 20), range(6), small, ext_st=[5, 7], dom=([7, 9], [20, 16]), core=([9, 10], [11, 9])))
    x, y = _grid((24, 20))
    c.append(Case("border_records", (24, 20), range(6), lambda t: ((x - 1.375) * (x - 12.625)) ** 2 / 64 + (y - (8.5 + 0.25 * t)) ** 2, dom=([1, 1], [22, 18])))
    # the smallest non-zero component is 1 / 256 to the bit: not BELOW 1 / hint, it leaves the running resolution alone
    c.append(Case("at_the_cap", (24, 20), range(6), with_value(rot, (1, 1, 0), 2.0 ** -8), nv=2))
    # the steps the context of keys_over sweeps while the one-launch pass sits out, and once more when it is back
    c.append(Case("keys_over_again", (132, 132), [4, 5], key_store_field(*KEYS_OVER_KNOBS[:3], extra=KEYS_OVER_KNOBS[3])))
    # ---- declines the kernel raises
    c.append(Case("inf", (24, 20), range(6), with_inf(small, 4, (3, 17)), expect=L["SERIES_INF"]))
    amb, _ = ambiguous_field((24, 20))
    c.append(Case("ambiguous", (24, 20), range(6), amb, nv=2, expect=L["SERIES_AMBIGUOUS"]))
    return {k.name: k for k in c}


# (a, b, q[, (row, column, height)]): found by a search over the family's knobs with the oracle, on the mesh the cases run on (domain = core =
# the vertices 2 .. 129, cells = 128 x 128): exactly kOneKeys keys in workgroup 85 and 1 770 records; exactly kOneKeys + 1 there and 1 764
# records.  No other workgroup parks more than 746.  tests/test_one_launch_cases.py holds both to these counts.
KEYS_FULL_KNOBS = (0.38, 0.66, 47)
KEYS_OVER_KNOBS = (0.22, 0.73, 63, (49, 96, 27.0))


def cases():
    if "cases" not in _cache:
        _cache["cases"] = _make_cases()
    return _cache["cases"]
