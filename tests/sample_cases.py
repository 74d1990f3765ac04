"""What tests/test_sample_steps_host.py and tests/test_gpu_aux.py share: the host build of ftk_amd/csrc/sample_steps.hpp
(tests/hostcheck/sample_host.cpp, a g++ shared object) as the oracle of the sample kernel, the meshes of the golden fixtures, the seeded
foreign fields and what the pinned CPU oracle (oracle/ftk_oracle.c, ftko_sweep) makes of them."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import golden_names, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "sample_host.cpp")
TAG_WORK_INDEX, TAG_REFERENCE, TAG_EXACT64 = 0, 1, 2
FOREIGN = ("random_2d_scalar_29x24x6", "random_2d_vector_23x20x5", "random_3d_scalar_13x12x11x4", "adversarial_3d_vector_8x8x8x3")
SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300])

_lib = None


def host(tmp_dir=None):
    """the shared object, built once per process"""
    global _lib
    if _lib is None:
        import tempfile
        so = os.path.join(str(tmp_dir) if tmp_dir is not None else tempfile.mkdtemp(prefix="hostcheck_sample"), "libhostcheck_sample.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", so, SRC])
        L = C.CDLL(so)
        vp = C.c_void_p
        L.hs_sample.argtypes = [C.c_int, vp, vp, vp, C.c_size_t, C.c_int, C.c_int, vp, vp, vp, vp, C.c_uint, C.c_int, vp, vp, vp]
        L.hs_sample.restype = C.c_size_t
        L.hs_element.argtypes = [C.c_int, vp, C.c_ulonglong, C.c_uint, vp, vp]
        L.hs_reference_ok.argtypes = [C.c_int, vp, C.c_int]
        _lib = L
    return _lib


def scalar_golden_names():
    """the fixtures that carry S"""
    return [n for n in golden_names() if not ("_vector_" in n or n.startswith("double_gyre"))]


def domain_of(g):
    """(starts, sizes) of the tracker's domain as the fixtures were made (json_interface.hh:634-656)"""
    scalar = g["nv"] == 1
    return [2 if scalar else 1] * g["nd"], [d - (3 if scalar else 2) for d in g["dims"]]


def mesh_ints(g, tag_mode):
    """the twenty ints of ftkx::SampleMesh for a fixture: core = domain, the array lattice starts at 0"""
    st, sz = domain_of(g)
    pad = lambda v, fill: list(v) + [fill] * (3 - len(v))          # noqa: E731
    return np.array([tag_mode, 1 if g["nv"] == 1 else 0] + pad(st, 0) + pad(sz, 1) + pad(st, 0) + pad(sz, 1) + [0, 0, 0] + pad(g["dims"], 1), dtype=np.int32)


def mesh_ints_of(tag_mode, scalar, dom, core, ext):
    """the twenty ints of ftkx::SampleMesh for any mesh: dom, core, ext = (starts, sizes) per spatial axis, as ftkx_set_mesh takes them"""
    pad = lambda v, fill: [int(x) for x in v] + [fill] * (3 - len(v))          # noqa: E731
    return np.array([tag_mode, 1 if scalar else 0] + pad(dom[0], 0) + pad(dom[1], 1) + pad(core[0], 0) + pad(core[1], 1) + pad(ext[0], 0) + pad(ext[1], 1), dtype=np.int32)


def aux_words(recs):
    """the aux word of include/ftkx.h from a record array with `ordinal` and `timestep`, or the one with `aux`"""
    if "aux" in recs.dtype.names:
        return np.ascontiguousarray(recs["aux"], dtype=np.uint32)
    return ((recs["timestep"].astype(np.uint32) << 1) | (recs["ordinal"].astype(np.uint32) & 1)).astype(np.uint32)


def work_index_tags(g, tags, aux):
    """element tags (64-bit) of a fixture -> the tags FTKX_TAG_WORK_INDEX gives the same elements: the corner's index inside core times
    the type count of the record's scope, plus the type's rank inside its scope"""
    nd = g["nd"]
    ntypes = 12 if nd == 2 else 60
    ordinal_types = [4, 8] if nd == 2 else [16, 20, 30, 34, 46, 50]
    interval_types = [t for t in range(ntypes) if t not in ordinal_types]
    _, sz = domain_of(g)
    cells = int(np.prod(sz, dtype=np.int64))
    tags = tags.astype(np.uint64)
    typ = (tags % np.uint64(ntypes)).astype(np.int64)
    lin = (tags // np.uint64(ntypes)).astype(np.int64) % cells           # (the time axis is the slowest: dropped)
    local = np.array([ordinal_types.index(t) if t in ordinal_types else interval_types.index(t) for t in typ], dtype=np.int64)
    n_scope = np.where(aux & 1, len(ordinal_types), len(interval_types)).astype(np.int64)
    return (lin * n_scope + local).astype(np.uint64)


def host_sample(g, tag_mode, tags, aux, A1=None, A2=None, t0=0, nthreads=1, fields=None, mesh=None):
    """hs_sample over a fixture's mesh and field arrays (fields: a list to take their place; mesh: the twenty ints of another mesh than the
    fixtures', mesh_ints_of).  A1 / A2: one array per timestep, or None.
    -> (slot 1 values or None, slot 2 values or None, ok flags, number of records that did not decode)"""
    L = host()
    steps = [np.ascontiguousarray(s, dtype=np.float64) for s in (fields if fields is not None else g["steps"])]
    n, nt = len(tags), len(steps)
    scalar = g["nv"] == 1

    def table(arrs):
        if arrs is None:
            return None, None
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
        return (C.c_void_p * nt)(*[None if a is None else a.ctypes.data for a in keep]), keep

    f_tab, f_keep = table(steps)
    a1, k1 = table(A1)
    a2, k2 = table(A2)
    tags = np.ascontiguousarray(tags, dtype=np.uint64)
    aux = np.ascontiguousarray(aux, dtype=np.uint32)
    o1 = np.full(n, 777.0) if A1 is not None else None
    o2 = np.full(n, 777.0) if A2 is not None else None
    ok = np.zeros(n, dtype=np.uint8)
    mesh = mesh_ints(g, tag_mode) if mesh is None else np.ascontiguousarray(mesh, dtype=np.int32)
    slots = (1 if A1 is not None else 0) | (2 if A2 is not None else 0)
    bad = L.hs_sample(g["nd"], mesh.ctypes.data, tags.ctypes.data, aux.ctypes.data, n, int(t0), nt, f_tab if scalar else None, None if scalar else f_tab, a1, a2, slots,
                      int(nthreads), None if o1 is None else o1.ctypes.data, None if o2 is None else o2.ctypes.data, ok.ctypes.data)
    return o1, o2, ok, int(bad)


def same_doubles(a, b):
    """bit patterns equal, a NaN equal to any NaN (which payload an operation hands on is the hardware's business)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def foreign_field(name, t, which=0):
    """B (which = 0) or C (1) of a case at timestep t: the extent of the fixture's S, uniform in +-10^3, every 17th value one of
    +-0.0, +-5e-324, +-1e300"""
    g = load_golden(name)
    shape = tuple(reversed(g["dims"]))
    seed = [FOREIGN.index(name) if name in FOREIGN else 99, int(t), int(which), 20240607]
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1e3, 1e3, size=shape)
    flat = b.reshape(-1)
    k = np.arange(0, flat.size, 17)
    flat[k] = SPECIALS[(np.arange(k.size) + int(t) + 3 * int(which)) % len(SPECIALS)]
    return b


_FOREIGN_CACHE = {}


def foreign_expectation(oracle, name, which=0):
    """{tag: scalar[0]} of ftko_sweep over the fixture's steps with S = the foreign field and the step's V, J and factor (64-bit element
    tags), both scopes of every step; computed once per process and handed out read-only"""
    key = (name, which)
    if key not in _FOREIGN_CACHE:
        g = load_golden(name)
        nd, nv, D, DT = g["nd"], g["nv"], g["dims"], g["DT"]
        dom = domain_of(g)
        VJ = []
        for a in g["steps"]:
            if nv == 1:
                V = oracle.gradient2D(a) if nd == 2 else oracle.gradient3D(a)
                J = oracle.jacobian2D(V, True) if nd == 2 else oracle.jacobian3D(V)
            else:
                V = a
                J = oracle.jacobian2D(a, False) if nd == 2 else oracle.jacobian3D(a)
            VJ.append((V, J))
        B = [foreign_field(name, t, which) for t in range(DT)]
        tags, vals = [], []
        for t in range(DT):
            for scope in (oracle.SCOPE_ORDINAL, oracle.SCOPE_INTERVAL):
                if scope == oracle.SCOPE_INTERVAL and t + 1 >= DT:
                    continue
                interval = scope == oracle.SCOPE_INTERVAL
                u = t + 1 if interval else t                     # (an ordinal sweep reads slice t alone)
                Vp, Jp, Sp = (VJ[t][0], VJ[u][0]), (VJ[t][1], VJ[u][1]), (B[t], B[u])
                r = oracle.sweep(nd, scope, t, dom, dom, ([0] * nd, D), Vp, Jp, Sp, int(g["factors"][t]), jacobian_symmetric=(nv == 1),
                                 robust=g["robust"], tag_mode=oracle.TAG_EXACT64, nthreads=4)
                tags.append(r["tag"]); vals.append(r["scalar"][:, 0])
        tags = np.concatenate(tags); vals = np.concatenate(vals)
        order = np.argsort(tags, kind="stable")
        tags, vals = tags[order], vals[order]
        assert len(np.unique(tags)) == len(tags)
        tags.setflags(write=False); vals.setflags(write=False)
        _FOREIGN_CACHE[key] = (tags, vals)
    return _FOREIGN_CACHE[key]


def expected_for(tags, expectation):
    """the oracle's value of every tag, record for record; the record set must be the oracle's"""
    etags, evals = expectation
    tags = np.ascontiguousarray(tags, dtype=np.uint64)
    assert len(tags) == len(etags) and np.array_equal(np.sort(tags), etags), "the record set is not the oracle's"
    return evals[np.searchsorted(etags, tags)]
