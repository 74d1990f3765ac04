"""Curve sets for the post-processing scans at the borders of their building block (post_process_kernels.hip): eight items per thread, 512
per wave, K = 2 048 per tile, 4K points per one-workgroup scan, 256 tiles = 524 288 points per batch of the spine.  Built directly as
(records, offsets, indices, loop) -- post-processing reads only type, aux and t of a record -- and GPU-free: the host function
ftkx_post_process_curves gives the expected result, tests/test_post_process_border_cases.py asserts what every set has to show, and the
GPU tests (tests/test_gpu_post_process_borders.py) and the steps' CPU check (tests/test_post_process_steps_host.py) run on the same sets.

Layouts:
  a  one curve
  b  curves of exactly 8, 512 and 2 048 points, each starting at a multiple of its own length (what is left over at the end: one short
     curve); besides the drawn ones an ordinal point at every multiple of 512 and a run head at every multiple of 2 048
  c  geometric lengths of mean 5 (a third of the curves have one point) with an empty curve in about every tenth place
  d  "head": geometric lengths of mean 50 with a curve's head at exactly point 524 288; "straddle": a curve that covers
     [524 288 - 4 096 - 1 234, 524 288 + 4 096 + 567).  That curve needs 4 096 points behind 524 288 and 257K + 1 has 2 049: the
     straddling set has 259K + 1 points (a size of its own, three tiles into the spine's second batch), and at 257K + 1 the curve runs
     from 524 288 - 4 096 - 1 234 to the end.  256K + 1 points end one point past 524 288: only "head" is built there (its last curve
     has one point)
  e  offsets[0] = 1 000 (the indices in front of it are -1: nobody may read them), twice as many records as points, indices a random
     injection

Values: types in runs along the curves as post_process_cases.scrambled() draws them (mean run length 1.3 / 4 / 30), ordinal bits with
probability 0.3, the timestep in aux from 4 values, t from {-0.0, 0.0, -0.25, 0.25, 0.5}, loop flags at random on curves of 3 points and
more.  Variants: "one_type" (type 2 everywhere: no split mode, every point kept, first = -1), "zero_type" (type 0 everywhere: split mode,
one run per curve), "no_ordinal", "all_ordinal".

Every set shows on the host result (shows_what_it_must; EXEMPT names what a variant excludes by construction): more trajectories than
curves, fewer points out than in, a changed type, a reversed piece, a rotated loop, and `t_tie` -- a t that comes out equal in value but
different in bits, -0.0 for 0.0 or the other way round: the tie on which std::max / std::min keep their first argument and a scan with
swapped operands would not.  A seed that does not show all of it is replaced by the next integer that does; SEEDS records them."""
import zlib

import numpy as np

from post_process_cases import TYPES

K = 2048
SPINE = 256 * K                                             # 524 288: one batch of the spine
SIZES = {"K-1": K - 1, "K": K, "K+1": K + 1, "2K-1": 2 * K - 1, "4K-1": 4 * K - 1, "4K": 4 * K, "4K+1": 4 * K + 1, "8K+1": 8 * K + 1,
         "256K": 256 * K, "256K+1": 256 * K + 1, "257K+1": 257 * K + 1, "259K+1": 259 * K + 1}
T_VALUES = np.array([-0.0, 0.0, -0.25, 0.25, 0.5])
EFFECTS = ("more_trajectories", "fewer_points", "type_changed", "reversed", "rotated", "t_tie")

# What a variant cannot show, by construction:
#   one_type, zero_type   one run per curve: nothing is cut or dropped, no type differs from the curve's first (no rotation), and smoothing
#                         between equal types changes none
#   no_ordinal            both smoothing steps work from the ordinal points: without them no type changes
#   all_ordinal           adjust_time leaves the t of an ordinal point alone: with every point ordinal no t changes, so there is no tie to
#                         keep either -- the one set without `t_tie`
EXEMPT = {"mixed": (), "one_type": ("more_trajectories", "fewer_points", "type_changed", "rotated"),
          "zero_type": ("more_trajectories", "fewer_points", "type_changed", "rotated"), "no_ordinal": ("type_changed",), "all_ordinal": ("t_tie",)}

# name -> (layout, size, mean run length, variant)
def _sets():
    s = {}
    for k, size in enumerate(SIZES):                        # (a) at every size, the run lengths in turn
        if size != "259K+1":
            s["a-%s" % size] = ("a", size, (1.3, 4, 30)[k % 3], "mixed")
    s["b-4K"] = ("b", "4K", 4, "mixed")
    s["b-8K+1"] = ("b", "8K+1", 30, "mixed")
    s["b-256K+1"] = ("b", "256K+1", 1.3, "mixed")
    s["c-4K+1"] = ("c", "4K+1", 1.3, "mixed")
    s["c-256K+1"] = ("c", "256K+1", 4, "mixed")
    s["c-257K+1"] = ("c", "257K+1", 1.3, "mixed")
    s["d-head-256K+1"] = ("d-head", "256K+1", 30, "mixed")
    s["d-head-257K+1"] = ("d-head", "257K+1", 4, "mixed")
    s["d-straddle-257K+1"] = ("d-straddle", "257K+1", 1.3, "mixed")
    s["d-straddle-259K+1"] = ("d-straddle", "259K+1", 1.3, "mixed")
    s["e-8K+1"] = ("e", "8K+1", 1.3, "mixed")
    s["e-256K+1"] = ("e", "256K+1", 30, "mixed")
    for v in ("one_type", "zero_type", "no_ordinal", "all_ordinal"):   # the variants: mid sizes in both forms of the scan, and once large
        s["c-4K+1-%s" % v] = ("c", "4K+1", 4, v)
        s["a-8K+1-%s" % v] = ("a", "8K+1", 1.3, v)
        s["c-257K+1-%s" % v] = ("c", "257K+1", 4, v)
    return s


SETS = _sets()

# Seeds: 0 wherever the set then shows what it must, otherwise the next integer that does (find_seed below).  The sets of one curve took
# some looking: to be rotated that curve has to be a loop between equal types, to be reversed it must not be a loop.
SEEDS = {name: 0 for name in SETS}
SEEDS.update({"a-K-1": 4, "a-K": 1, "a-K+1": 8, "a-2K-1": 1, "a-4K-1": 3, "a-4K": 3, "a-4K+1": 6, "a-8K+1": 7, "a-256K": 2, "a-256K+1": 11, "a-257K+1": 36,
              "b-4K": 1, "a-8K+1-one_type": 1, "a-8K+1-no_ordinal": 1, "a-8K+1-all_ordinal": 7})

# Kept-count borders: the points that ScanTimeForward / ScanTimeBackward run over are the M kept ones, on a grid sized by np.  A mixed
# set of layout (c) with fewer than M kept points, and behind it curves of one non-zero type -- every point of those is kept -- to make M
# exact.  name -> (np of the mixed part, mean run length, M).  M = 4K with np > 4K: a scan in three launches over what one workgroup
# would take, ending on a tile's border.
KEPT = {"kept-4K": (4 * K + 301, 1.3, 4 * K), "kept-4K+1": (4 * K + 301, 4, 4 * K + 1), "kept-6K": (6 * K - 1, 4, 6 * K)}
SEEDS.update({name: 0 for name in KEPT})

LARGE = [n for n, s in SETS.items() if SIZES[s[1]] >= 256 * K]
ALL = list(SETS) + list(KEPT)


def _lengths(layout, n, rng):
    """the curves' lengths in order (0: an empty curve)"""
    if layout == "a":
        return np.array([n], dtype=np.int64)
    if layout == "b":
        out, pos = [2048, 512, 8], 2048 + 512 + 8            # one of each, then as they come: the longest that fits here, or a shorter one
        while n - pos >= 8:
            fit = [L for L in (2048, 512, 8) if pos % L == 0 and pos + L <= n]
            L = fit[0] if rng.random() < 0.5 else fit[int(rng.integers(0, len(fit)))]
            out.append(L)
            pos += L
        if pos < n:
            out.append(n - pos)
        return np.array(out, dtype=np.int64)

    def geometric(total, mean):
        if total <= 0:
            return np.zeros(0, dtype=np.int64)
        ln = rng.geometric(1.0 / mean, size=int(total / mean * 1.5) + 64)
        cs = np.cumsum(ln)
        assert cs[-1] >= total
        m = int(np.searchsorted(cs, total))
        ln = ln[:m + 1].copy()
        ln[m] -= cs[m] - total
        return ln.astype(np.int64)
    if layout in ("c", "e"):
        ln = geometric(n, 5)
        empty = rng.random(len(ln) + 1) < 0.1                # an empty curve in front of about every tenth, and perhaps one at the end
        out = np.zeros(len(ln) + int(empty.sum()), dtype=np.int64)
        place = np.arange(len(ln)) + np.cumsum(empty[:-1])
        out[place] = ln
        return out
    if layout == "d-head":
        return np.concatenate([geometric(SPINE, 50), geometric(n - SPINE, 50)])
    if layout == "d-straddle":
        b, e = SPINE - 4096 - 1234, min(SPINE + 4096 + 567, n)
        assert e - SPINE >= 4096 or n == SIZES["257K+1"]
        return np.concatenate([geometric(b, 50), [e - b], geometric(n - e, 50)])
    raise ValueError(layout)


def _values(recs, flat, heads, n, run_length, variant, rng, forced=False):
    """type, aux and t of the n points' records; heads: the positions at which curves start"""
    lengths = rng.geometric(1.0 / run_length, size=n + 1)   # runs along the flat point array, cut at the curves' heads
    starts = np.concatenate([[0], np.cumsum(lengths)])
    starts = starts[starts < n]
    run_of = np.zeros(n, dtype=np.int64)
    run_of[starts] = 1
    run_of[heads[heads < n]] = 1
    if forced:
        run_of[::K] = 1
    run_of = np.cumsum(run_of) - 1
    types = TYPES[rng.integers(0, len(TYPES), size=int(run_of[-1]) + 1)]
    ty = types[run_of]
    ordinal = (rng.random(n) < 0.3).astype(np.uint32)
    if forced:
        ordinal[::512] = 1
    if variant == "one_type":
        ty = np.full(n, 2, dtype=np.uint32)
    elif variant == "zero_type":
        ty = np.zeros(n, dtype=np.uint32)
    elif variant == "no_ordinal":
        ordinal[:] = 0
    elif variant == "all_ordinal":
        ordinal[:] = 1
    recs["type"][flat] = ty
    recs["aux"][flat] = (rng.integers(0, 4, size=n).astype(np.uint32) << 1) | ordinal
    recs["t"][flat] = T_VALUES[rng.integers(0, len(T_VALUES), size=n)]


def build(name, seed=None):
    """-> (records, offsets, indices, loop): curve c is indices[offsets[c]:offsets[c + 1]] into records"""
    import ftk_amd
    seed = SEEDS[name] if seed is None else seed
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    if name in KEPT:
        return _build_kept(name, rng)
    layout, size, run_length, variant = SETS[name]
    n = SIZES[size]
    ln = _lengths(layout, n, rng)
    assert ln.sum() == n
    first = 1000 if layout == "e" else 0
    offs = first + np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    n_rec = 2 * n if layout == "e" else n
    flat = rng.permutation(n_rec)[:n].astype(np.int64)
    recs = np.zeros(n_rec, dtype=ftk_amd.CP_DTYPE)
    if layout == "e":                                       # the records no curve uses: anything
        recs["type"] = TYPES[rng.integers(0, len(TYPES), size=n_rec)]
        recs["t"] = rng.uniform(-1, 1, size=n_rec)
        recs["aux"] = rng.integers(0, 16, size=n_rec).astype(np.uint32)
    _values(recs, flat, offs[:-1] - first, n, run_length, variant, rng, forced=layout == "b")
    loop = ((ln >= 3) & (rng.random(len(ln)) < 0.5)).astype(np.int32)
    indices = np.concatenate([np.full(first, -1, dtype=np.int64), flat])
    return recs, offs, indices, loop


def _build_kept(name, rng):
    import ftk_amd
    n0, run_length, M = KEPT[name]
    ln = _lengths("c", n0, rng)
    recs0 = np.zeros(n0, dtype=ftk_amd.CP_DTYPE)
    flat0 = rng.permutation(n0).astype(np.int64)
    offs0 = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    _values(recs0, flat0, offs0[:-1], n0, run_length, "mixed", rng)
    loop0 = ((ln >= 3) & (rng.random(len(ln)) < 0.5)).astype(np.int32)
    M0 = len(ftk_amd.post_process_curves(recs0, offs0, flat0, loop0).indices)
    assert M0 < M, (name, M0)
    # behind them: curves of type 4 throughout, M - M0 points in all, in three curves where there are enough
    extra = M - M0
    cut = [extra] if extra < 9 else [extra // 3, extra // 3, extra - 2 * (extra // 3)]
    recs1 = np.zeros(extra, dtype=ftk_amd.CP_DTYPE)
    recs1["type"] = 4
    recs1["aux"] = (rng.integers(0, 4, size=extra).astype(np.uint32) << 1) | (rng.random(extra) < 0.3).astype(np.uint32)
    recs1["t"] = T_VALUES[rng.integers(0, len(T_VALUES), size=extra)]
    recs = np.concatenate([recs0, recs1])
    offs = np.concatenate([offs0, n0 + np.cumsum(cut)]).astype(np.int64)
    indices = np.concatenate([flat0, n0 + np.arange(extra)]).astype(np.int64)
    loop = np.concatenate([loop0, (rng.random(len(cut)) < 0.5).astype(np.int32)]).astype(np.int32)
    return recs, offs, indices, loop


def variant_of(name):
    return "mixed" if name in KEPT else SETS[name][3]


def effects(recs, offs, indices, loop, ts):
    """which effects of the post-processing the trajectories `ts` (host result) show: those of post_process_cases.effects on curves
    given as arrays, and t_tie"""
    first, end = int(offs[0]), int(offs[-1])
    where = np.full(len(recs), -1, dtype=np.int64)          # record -> position in the flat point array
    where[indices[first:end]] = np.arange(first, end)
    curve_of = np.full(end, -1, dtype=np.int64)
    curve_of[first:] = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    t_in = recs["t"][ts.indices]
    e = {"more_trajectories": len(ts) > len(offs) - 1, "fewer_points": len(ts.indices) < end - first,
         "type_changed": bool(np.any(ts.type != recs["type"][ts.indices])),
         "t_tie": bool(np.any((ts.t == t_in) & (ts.t.view(np.uint64) != t_in.view(np.uint64)))),
         "reversed": False, "rotated": False}
    pos = where[ts.indices]
    assert np.all(pos >= first)
    assert np.array_equal(curve_of[pos], np.repeat(ts.id, np.diff(ts.offsets)))
    a, b = ts.offsets[:-1], ts.offsets[1:]
    c = ts.id.astype(np.int64)
    n = offs[c + 1] - offs[c]
    two = (b - a >= 2) & (n >= 3)
    step = (pos[np.minimum(a + 1, len(pos) - 1)] - pos[np.minimum(a, len(pos) - 1)]) if len(pos) else np.zeros(len(a), dtype=np.int64)
    e["reversed"] = bool(np.any(two & (step % np.maximum(n, 1) == n - 1)))
    # the first piece of a curve: without a rotation it holds the curve's first point
    firsts = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]])) if len(c) else np.zeros(0, dtype=np.int64)
    for k in firsts[(loop[c[firsts]] != 0) & (b[firsts] > a[firsts])]:
        if not np.any(pos[a[k]:b[k]] == offs[c[k]]):
            e["rotated"] = True
            break
    return e


def shows_what_it_must(name, recs, offs, indices, loop, ts):
    e = effects(recs, offs, indices, loop, ts)
    exempt = EXEMPT[variant_of(name)]
    for f in exempt:
        assert not e[f], (name, f, "excluded by construction, yet seen")
    return all(e[f] for f in EFFECTS if f not in exempt)


def find_seed(name, start=0):
    """the first seed from `start` on with which the set shows what it must (for whoever adds a set: write it into SEEDS)"""
    import ftk_amd
    for seed in range(start, start + 200):
        recs, offs, indices, loop = build(name, seed)
        if shows_what_it_must(name, recs, offs, indices, loop, ftk_amd.post_process_curves(recs, offs, indices, loop)):
            return seed
    raise AssertionError(name)


_cache = {}


def case(name):
    """-> (records, offsets, indices, loop, host trajectories); built once per process for the small sets, never changed.  The large
    sets (38 MB of records each) are built anew: keeping a dozen of them would cost half a gigabyte"""
    import ftk_amd
    if name in _cache:
        return _cache[name]
    recs, offs, indices, loop = build(name)
    host = ftk_amd.post_process_curves(recs, offs, indices, loop)
    for a in (recs, offs, indices, loop):
        a.setflags(write=False)
    out = (recs, offs, indices, loop, host)
    if name not in LARGE:
        _cache[name] = out
    return out
