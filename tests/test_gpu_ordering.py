"""The two hand-written ordering paths at the COUNTS where their branches open, on series small enough for the suite.

The bucket chain of the device-driven pass (series_kernels.hip: bucket_scan_kernel<4|16>, bucket_scatter_kernel, bucket_rank_kernel, and
the host's repair behind SERIES_FIX_ORDER, series_order.hpp) spreads the keys over 2^14 buckets whatever the series: a small series never
fills a bucket.  FTKX_SERIES_HOOKS bins=K makes it 2^K buckets, and two rough fields on a 1/64 grid (factor 256, no overflow regime, many
ties) then reach: buckets of hundreds and thousands staged in LDS, a workgroup's span past the 4 096 keys LDS holds (ranked from global
memory), buckets at rank_max to the key, passes where the device ranks some buckets and the host repairs others, a single bucket, fewer
buckets than the scan has wavefronts, and all of it through the split form.  Every case reads ftkx_debug_series_order and the status bits
and asserts that it reached the branch it names: a case that silently ran the default geometry fails.  The reference is the oracle's
track under TAG_EXACT64, stably sorted by tag; records are compared bit for bit and IN ORDER.

The radix sort of the host-driven batch (collect.hip: rs_count_kernel, rs_scan_kernel, rs_scatter_kernel, sort_gather_kernel) through
ftkx_debug_sort_records -- the production sort_hits_on_device on records made here -- against numpy's stable argsort, as bytes: n at the
tile borders (2 048 keys), at the 4 096 where ftkx_sweep_collect starts to use it, where the scan's per-thread share goes from 1 to 2
counts (131 072 records), both parities of the number of digit passes (the ping-pong half the gather reads), stability, a tile whose
keys all share a digit (a column prefix of 2 048 in 16 bits), bit 63.  And one end-to-end batch over 64 tiles against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from common import assert_records_equal

pytestmark = pytest.mark.gpu

FIX_ORDER = 16                          # SERIES_FIX_ORDER
NOT_DEVICE_DRIVEN = 1 | 2 | 4 | 8 | 256    # SERIES_AMBIGUOUS, _MASKS_INVALID, _INF, _OVERFLOW, _HALO_FULL: the host-driven batch took the pass over
SPAN = 4096                             # keys of a workgroup's span that bucket_rank_kernel stages in LDS; rank_max's default is the same number
D2 = ((64, 48), 4)
D3 = ((40, 36, 20), 3)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


def _rough(dims, nt):
    rng = np.random.default_rng(7)
    shape = tuple(reversed(dims))
    return [np.round(rng.standard_normal(shape) * 2) * 0.25 + rng.integers(-2, 3, size=shape) / 64.0 for _ in range(nt)]


_CACHE = {}


def _data(oracle, which, tag_mode=None):
    """(steps, the oracle's records stably sorted by tag, its factors): computed once per series and tag mode, never changed"""
    tag_mode = oracle.TAG_EXACT64 if tag_mode is None else tag_mode
    key = (which, tag_mode)
    if key not in _CACHE:
        dims, nt = which
        if (which, "steps") not in _CACHE:
            _CACHE[(which, "steps")] = _rough(dims, nt)
        steps = _CACHE[(which, "steps")]
        ref, rf, _ = oracle.track(steps, len(dims), 1, tag_mode=tag_mode, nthreads=min(8, os.cpu_count() or 1))
        ref = ref[np.argsort(ref["tag"], kind="stable")]
        ref.setflags(write=False)
        _CACHE[key] = (steps, ref, [int(f) for f in rf])
    return _CACHE[key]


def _ctx(gpu, dims, tag_mode):
    nd = len(dims)
    dom = ([2] * nd, [d - 3 for d in dims])
    ctx = gpu.Context(nd)
    ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
    ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=tag_mode)
    return ctx


def _as_fixture(recs):
    out = np.zeros(len(recs), dtype=[("tag", "<u8"), ("type", "<u4"), ("ordinal", "<i4"), ("timestep", "<i4"), ("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,))])
    for f in ("tag", "type", "x", "t", "scalar"):
        out[f] = recs[f]
    out["ordinal"] = recs["aux"] & 1
    out["timestep"] = recs["aux"] >> 1
    return out


def _assert_in_order_and_equal(recs, ref, what):
    """the records as they came, position by position (assert_records_equal alone would sort them first)"""
    assert len(recs) == len(ref), f"{what}: {len(recs)} records, expected {len(ref)}"
    bad = np.flatnonzero(recs["tag"] != ref["tag"])
    assert bad.size == 0, f"{what}: {bad.size} records out of tag order, the first at {int(bad[0])} of {len(ref)}"
    assert_records_equal(_as_fixture(recs), ref, coord_tol=0.0, what=what)


def _bucket_sizes(ref, nd, shift):
    """records per bucket of the ordering step, from the reference's element tags: order key = (element << 6) | type"""
    per = 12 if nd == 2 else 60
    tag = ref["tag"].astype(np.uint64)
    key = ((tag // np.uint64(per)) << np.uint64(6)) | (tag % np.uint64(per))
    return np.bincount((key >> np.uint64(shift)).astype(np.int64))


def _widest_span(sizes):
    """the widest span of bucket_rank_kernel's workgroups: 256 consecutive positions, from the start of the first one's bucket to the end of the last one's"""
    boff = np.concatenate([[0], np.cumsum(sizes)])
    count = int(boff[-1])
    first = np.arange(0, count, 256)
    last = np.minimum(first + 255, count - 1)
    b0 = np.searchsorted(boff, first, side="right") - 1
    b1 = np.searchsorted(boff, last, side="right") - 1
    return int((boff[b1 + 1] - boff[b0]).max())


def _chain_pass(gpu, oracle, which, hooks, monkeypatch, what):
    """one pass of the kernel chain over the series under FTKX_SERIES_HOOKS one=0,small=0,<hooks> -> (records, ftkx_debug_series_order,
    status, reference).  A series with more records than the default hit buffer is swept again on the context that has grown, and that pass
    is the one returned."""
    steps, ref, rf = _data(oracle, which)
    dims, nt = which
    monkeypatch.setenv("FTKX_SERIES_HOOKS", "one=0,small=0" + ("," + hooks if hooks else ""))
    ctx = _ctx(gpu, dims, gpu.TAG_EXACT64)
    for t, a in enumerate(steps):
        ctx.push_scalar_slice(t, a)
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    recs, f, _ = ctx.sweep_series(range(nt), scopes)
    grown = 0
    while ctx.series_last_path()[0] == 0 and len(ref) > 65536 and grown < 2:      # (the buffers grow by what the pass counted: once, twice where a list was cut short)
        assert ctx.series_order() == dict(nbins=0, shift=0, fullest=0, rank_max=0), what
        recs, f, _ = ctx.sweep_series(range(nt), scopes)
        grown += 1
    path, status = ctx.series_last_path()
    order = ctx.series_order()
    ctx.close()
    print(what, "path", path, "status", status, order, "records", len(recs), "sweeps", 1 + grown)
    assert path == 1 and not (status & NOT_DEVICE_DRIVEN), f"{what}: path {path}, status {status}"
    assert [int(v) for v in f] == rf and set(rf) == {256}, (what, f, rf)
    _assert_in_order_and_equal(recs, ref, what)
    return recs, order, status, ref


def _assert_geometry(order, bins, what):
    assert order["nbins"] <= (1 << bins) and (bins == 0 or order["nbins"] > (1 << bins) // 2), f"{what}: {order} is not the geometry of bins={bins}"


# ---- the bucket chain ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [D2, D3], ids=["2d", "3d"])
def test_fat_buckets_staged_in_lds(gpu, oracle, monkeypatch, which):
    """bins=8: buckets of hundreds (2D) and thousands (3D) of keys, none past rank_max: all ranked on the device"""
    what = f"staged, fat buckets, {len(which[0])}D"
    recs, o, status, ref = _chain_pass(gpu, oracle, which, "bins=8", monkeypatch, what)
    _assert_geometry(o, 8, what)
    assert 100 <= o["fullest"] <= SPAN and o["rank_max"] == 4096 and not (status & FIX_ORDER), (what, o, status)


def test_span_wider_than_lds_ranked_from_global_memory(gpu, oracle, monkeypatch):
    """2D bins=4: no bucket past rank_max, two neighbours together past SPAN -- a workgroup whose 256 positions straddle them ranks out of bucketed[]"""
    what = "unstaged, ranked"
    recs, o, status, ref = _chain_pass(gpu, oracle, D2, "bins=4", monkeypatch, what)
    _assert_geometry(o, 4, what)
    sizes = _bucket_sizes(ref, 2, o["shift"])
    assert len(sizes) <= o["nbins"] and int(sizes.max()) == o["fullest"], (what, o, int(sizes.max()))
    assert o["fullest"] <= SPAN < int((sizes[1:] + sizes[:-1]).max()) and _widest_span(sizes) > SPAN, (what, o, sizes.tolist(), _widest_span(sizes))
    assert o["rank_max"] == 4096 and not (status & FIX_ORDER), (what, o, status)


def test_some_buckets_ranked_on_the_device_others_repaired_by_the_host(gpu, oracle, monkeypatch):
    what = "mixed"
    recs, o, status, ref = _chain_pass(gpu, oracle, D2, "bins=3", monkeypatch, what)
    _assert_geometry(o, 3, what)
    sizes = _bucket_sizes(ref, 2, o["shift"])
    assert int(sizes.max()) == o["fullest"] > o["rank_max"] == 4096 and (status & FIX_ORDER), (what, o, status)
    assert np.any((sizes > 1) & (sizes <= o["rank_max"])) and np.any(sizes > o["rank_max"]), (what, sizes.tolist())


def test_rank_max_to_the_key(gpu, oracle, monkeypatch):
    """the fullest bucket holds F keys: with rank_max=F the device ranks it, with rank_max=F-1 the host does"""
    _, o, _, _ = _chain_pass(gpu, oracle, D2, "bins=8", monkeypatch, "rank_max border, first run")
    F = o["fullest"]
    assert F >= 100, o
    _, o, status, _ = _chain_pass(gpu, oracle, D2, f"bins=8,rank_max={F}", monkeypatch, "rank_max = F")
    assert o["fullest"] == F == o["rank_max"] and not (status & FIX_ORDER), (o, status)
    _, o, status, _ = _chain_pass(gpu, oracle, D2, f"bins=8,rank_max={F - 1}", monkeypatch, "rank_max = F - 1")
    assert o["fullest"] == F == o["rank_max"] + 1 and (status & FIX_ORDER), (o, status)


def test_one_bucket(gpu, oracle, monkeypatch):
    """bins=0: every key in one bucket -- repaired by the host as a whole, or (rank_max=30000) ranked on the device out of global memory"""
    recs, o, status, ref = _chain_pass(gpu, oracle, D2, "bins=0", monkeypatch, "one bucket, host")
    assert o == dict(nbins=1, shift=o["shift"], fullest=len(ref), rank_max=4096) and len(ref) > SPAN and (status & FIX_ORDER), (o, status)
    recs, o, status, ref = _chain_pass(gpu, oracle, D2, "bins=0,rank_max=30000", monkeypatch, "one bucket, device")
    assert o == dict(nbins=1, shift=o["shift"], fullest=len(ref), rank_max=30000) and SPAN < len(ref) <= 30000 and not (status & FIX_ORDER), (o, status)


@pytest.mark.parametrize("bins", [1, 2])
def test_fewer_buckets_than_the_scan_has_wavefronts(gpu, oracle, monkeypatch, bins):
    what = f"bins={bins}"
    recs, o, status, ref = _chain_pass(gpu, oracle, D2, f"bins={bins}", monkeypatch, what)
    _assert_geometry(o, bins, what)
    assert o["nbins"] == 2 if bins == 1 else 2 < o["nbins"] <= 4, o
    sizes = _bucket_sizes(ref, 2, o["shift"])
    assert int(sizes.max()) == o["fullest"] and bool(status & FIX_ORDER) == (o["fullest"] > 4096), (o, status)


@pytest.mark.parametrize("bins", [8, 3])
def test_split_form(gpu, oracle, monkeypatch, bins):
    """ftkx_sweep_series_submit / _complete under split=2: path 5 -- bucket_scan_kernel<4>, the records by way of the copy kernel; bins=3:
    the host repairs records that came through series_copy_out_kernel"""
    steps, ref, rf = _data(oracle, D2)
    dims, nt = D2
    monkeypatch.setenv("FTKX_SERIES_HOOKS", f"one=0,small=0,split=2,bins={bins}")
    ctx = _ctx(gpu, dims, gpu.TAG_EXACT64)
    for t, a in enumerate(steps):
        ctx.push_scalar_slice(t, a)
    scopes = [gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL for t in range(nt)]
    want, wf, _ = ctx.sweep_series(range(nt), scopes)               # (not pipelined: in order; the passes behind it know the record count)
    assert ctx.series_last_path()[0] == 1
    _assert_in_order_and_equal(want, ref, f"split form bins={bins}, the plain pass")
    ctx.invalidate_masks()
    ctx.sweep_series_submit(range(nt), scopes)
    ctx.invalidate_masks()
    ctx.sweep_series_submit(range(nt), scopes)
    for k in range(2):
        got, f, _ = ctx.sweep_series_complete()
        path, status = ctx.series_last_path()
        o = ctx.series_order()
        what = f"split form bins={bins}, pass {k}"
        print(what, "path", path, "status", status, o)
        assert path == 5 and not (status & NOT_DEVICE_DRIVEN), (what, path, status)
        _assert_geometry(o, bins, what)
        assert bool(status & FIX_ORDER) == (bins == 3) and (o["fullest"] > 4096) == (bins == 3) and o["fullest"] >= 100 and o["rank_max"] == 4096, (what, o, status)
        assert [int(v) for v in f] == rf
        _assert_in_order_and_equal(got, ref, what)
    ctx.close()


def test_3d_default_geometry(gpu, oracle, monkeypatch):
    """no bins hook: 295 667 records through 2^14 buckets on a context whose buffers have grown"""
    what = "3D, default geometry"
    recs, o, status, ref = _chain_pass(gpu, oracle, D3, "", monkeypatch, what)
    assert len(ref) > 65536
    assert (1 << 13) < o["nbins"] <= (1 << 14) and 1 <= o["fullest"] <= 4096 and o["rank_max"] == 4096 and not (status & FIX_ORDER), (what, o, status)
    sizes = _bucket_sizes(ref, 3, o["shift"])
    assert int(sizes.max()) == o["fullest"], (what, o, int(sizes.max()))


# ---- the radix sort --------------------------------------------------------------------------------------------------------------------

NS = [1, 2, 255, 2047, 2048, 2049, 4095, 4096, 4097, 131071, 131072, 131073, 262145]      # 131 072 = 64 tiles: 1 024 counts, a count per thread of the scan; one more: two
KEY_BITS = [1, 4, 5, 8, 33, 60, 63, 64]        # digit passes: 1, 1, 2, 2, 9, 15, 16, 16
PATTERNS = ["uniform", "sorted", "descending", "all_equal", "three_values", "tile_in_one_digit", "bit63"]


def _tags(pattern, n, key_bits, rng):
    mask = np.uint64((1 << key_bits) - 1)
    uniform = np.frombuffer(rng.bytes(8 * n), dtype="<u8") & mask
    if pattern == "uniform":
        return uniform
    if pattern == "sorted":
        return np.sort(uniform)
    if pattern == "descending":
        return np.sort(uniform)[::-1].copy()
    if pattern == "all_equal":
        return np.full(n, uniform[0], dtype=np.uint64)
    if pattern == "three_values":
        vals = np.unique(np.array([0, int(mask) >> 1, int(mask)], dtype=np.uint64))
        return vals[rng.integers(0, len(vals), size=n)]
    if pattern == "tile_in_one_digit":      # input tile j: the same digit, j % 16, in every place -- the first pass's column prefixes run to the tile's 2 048 keys
        return (((np.arange(n, dtype=np.uint64) // np.uint64(2048)) % np.uint64(16)) * np.uint64(0x1111111111111111)) & mask
    if pattern == "bit63":
        assert key_bits == 64
        return uniform | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    raise ValueError(pattern)


def _records(gpu, tags, rng):
    """every word of a record but the tag from the generator: a gather that mixes up the nine words of a record, or two records, shows"""
    r = np.frombuffer(rng.bytes(gpu.CP_DTYPE.itemsize * len(tags)), dtype=gpu.CP_DTYPE).copy()
    r["tag"] = tags
    return r


_SORT_CASES = ([(n, kb, p) for n in NS for kb in (33, 64) for p in ("uniform", "three_values")] +
               [(n, kb, p) for n in (4097, 131073) for kb in KEY_BITS for p in PATTERNS if p != "bit63" or kb == 64])
_SORT_CASES = sorted(set(_SORT_CASES), key=lambda c: (c[0], c[1], PATTERNS.index(c[2])))


@pytest.fixture(scope="module")
def sort_ctx(gpu):
    ctx = gpu.Context(2)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n,key_bits,pattern", _SORT_CASES, ids=[f"n{n}-bits{kb}-{p}" for n, kb, p in _SORT_CASES])
def test_radix_sort_is_a_stable_sort(gpu, sort_ctx, n, key_bits, pattern):
    rng = np.random.default_rng([n, key_bits, PATTERNS.index(pattern)])
    tags = _tags(pattern, n, key_bits, rng)
    assert tags.dtype == np.uint64 and len(tags) == n and (key_bits == 64 or int(tags.max()) < (1 << key_bits))
    recs = _records(gpu, tags, rng)
    want = recs[np.argsort(recs["tag"], kind="stable")]
    if pattern == "all_equal":
        assert want.tobytes() == recs.tobytes()
    got = sort_ctx.debug_sort_records(recs, key_bits)
    if got.tobytes() != want.tobytes():
        wrong = np.flatnonzero(got["tag"] != want["tag"])
        moved = np.flatnonzero(np.any(got.view(np.uint64).reshape(n, 9) != want.view(np.uint64).reshape(n, 9), axis=1))
        raise AssertionError(f"n {n} key_bits {key_bits} {pattern}: {wrong.size} tags out of place, {moved.size} records differ, the first at {int(moved[0])}")


@pytest.mark.parametrize("mode", ["exact64", "reference"])
def test_batched_3d_collect_against_the_oracle(gpu, oracle, mode):
    """every sweep of the 3D series enqueued, one collect: 295 667 records -- 145 tiles -- through the device sort, under element tags
    (key_bits from the mesh) and under the reference's tags (64 key bits), against the oracle"""
    from ftk_amd import tslab
    tag_mode, otag = (gpu.TAG_EXACT64, oracle.TAG_EXACT64) if mode == "exact64" else (gpu.TAG_REFERENCE, oracle.TAG_REFERENCE)
    steps, ref, rf = _data(oracle, D3, otag)
    dims, nt = D3
    ctx = _ctx(gpu, dims, tag_mode)
    res = []
    for t in range(nt):
        ctx.push_scalar_slice(t, steps[t])
        res.append(ctx.slice_resolution(t)[0])
    factors = tslab.factors_from_resolutions(res)
    for t in range(nt):
        ctx.sweep_enqueue(t, gpu.SCOPE_BOTH if t + 1 < nt else gpu.SCOPE_ORDINAL, factors[t])
    recs = ctx.sweep_collect()
    ctx.close()
    assert [int(f) for f in factors] == rf
    assert len(ref) > 64 * 2048
    _assert_in_order_and_equal(recs, ref, f"batched 3D collect, {mode} tags")


# ---- the two entries' argument errors ----------------------------------------------------------------------------------------------------

def test_argument_errors_start_nothing(gpu, sort_ctx):
    from ftk_amd import _lib
    L = _lib.load()
    E = _lib.E_INVALID
    one = _records(gpu, np.array([5], dtype=np.uint64), np.random.default_rng(1))
    out = np.zeros_like(one)
    o4 = (C.c_ulonglong * 4)(7, 7, 7, 7)
    assert L.ftkx_debug_series_order(None, o4) == E and list(o4) == [7, 7, 7, 7]
    assert L.ftkx_debug_series_order(sort_ctx._h, None) == E
    assert L.ftkx_debug_series_order(sort_ctx._h, o4) == 0 and list(o4) == [0, 0, 0, 0]      # (no series pass yet)
    assert L.ftkx_debug_sort_records(None, one.ctypes.data, 1, 8, out.ctypes.data) == E
    for bits in (0, -1, 65, 1 << 20):
        assert L.ftkx_debug_sort_records(sort_ctx._h, one.ctypes.data, 1, bits, out.ctypes.data) == E, bits
    assert L.ftkx_debug_sort_records(sort_ctx._h, None, 1, 8, out.ctypes.data) == E
    assert L.ftkx_debug_sort_records(sort_ctx._h, one.ctypes.data, 1, 8, None) == E
    assert not out.view(np.uint8).any()                                                      # (nothing was written)
    assert L.ftkx_debug_sort_records(sort_ctx._h, None, 0, 8, None) == 0                      # no records: nothing to do
    assert len(sort_ctx.debug_sort_records(one[:0], 64)) == 0
    with pytest.raises(gpu.FtkxError):
        sort_ctx.debug_sort_records(one, 0)
    assert sort_ctx.debug_sort_records(one, 8).tobytes() == one.tobytes()                     # the context is as good as before
