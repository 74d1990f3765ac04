"""Inputs for tests/test_gpu_post_process_device.py, built the same way by the test and by whoever checks its seeds on a CPU (the host
function ftkx_post_process_curves needs no GPU).

The fixtures' own records reach every branch of the post-processing somewhere (merger: smoothed ordinal types, mixed gaps, rotations,
splits, reversals; singular_terraces: the same by the dozen, and hundreds of curves without ordinal points; the overflow fixture: no
ordinal point at all and 15 309 curves of one point), but some of them only a few times.  The scrambled sets make them common: along every
traced curve the types are drawn again in runs, the ordinal bits with probability 0.3, and t is jittered."""
import numpy as np

from trace_device_cases import FIXTURES, fixture_records  # noqa: F401

SCRAMBLED_FIXTURES = ["woven_31x37x32", "singular_terraces_72x64x56x8"]
RUN_LENGTHS = [1.3, 4, 30]
TYPES = np.array([0, 1, 2, 4, 8], dtype=np.uint32)

# Per (fixture, mean run length) eight seeds.  With each of them the host result shows every effect (shows_every_effect; the test asserts
# it again): more trajectories than curves, fewer points out than in, a changed type, a changed t, a reversed piece and -- where the
# fixture has a loop curve that can be rotated at all, see can_rotate -- a loop curve that starts elsewhere.  For run length 1.3 the drawn
# types also hold three maximal runs of length 1 in a row behind a longer run (the alternating drop of split_all).  Seeds 0..7 wherever
# they do; a seed that does not would be replaced by the next integer that does (none had to be).
SCRAMBLE_SEEDS = {
    ("woven_31x37x32", 1.3): [0, 1, 2, 3, 4, 5, 6, 7],
    ("woven_31x37x32", 4): [0, 1, 2, 3, 4, 5, 6, 7],
    ("woven_31x37x32", 30): [0, 1, 2, 3, 4, 5, 6, 7],
    ("singular_terraces_72x64x56x8", 1.3): [0, 1, 2, 3, 4, 5, 6, 7],
    ("singular_terraces_72x64x56x8", 4): [0, 1, 2, 3, 4, 5, 6, 7],
    ("singular_terraces_72x64x56x8", 30): [0, 1, 2, 3, 4, 5, 6, 7],
}

_curves = {}


def traced(name):
    """-> (offsets, flat indices, loop flags) of the fixture's traced curves (host trace); computed once, never changed"""
    import ftk_amd
    if name not in _curves:
        g, dom, recs = fixture_records(name)
        curves, loop, _ = ftk_amd.trace_curves(g["nd"], dom, recs)
        offs = np.concatenate([[0], np.cumsum([len(c) for c in curves])]).astype(np.int64)
        flat = np.concatenate(curves).astype(np.int64) if len(curves) else np.zeros(0, np.int64)
        for a in (offs, flat):
            a.setflags(write=False)
        _curves[name] = (offs, flat, np.asarray(loop, dtype=np.int32))
    return _curves[name]


def scrambled(name, run_length, seed):
    """the fixture's records with type, ordinal bit and t drawn again along its traced curves (tags untouched: the same curves)"""
    g, dom, recs = fixture_records(name)
    offs, flat, _ = traced(name)
    rng = np.random.default_rng([seed, int(round(run_length * 10)), SCRAMBLED_FIXTURES.index(name)])
    out = recs.copy()
    n = len(flat)
    # runs along the flat point array, cut at the curves' heads: lengths geometric with the given mean
    lengths = rng.geometric(1.0 / run_length, size=n + 1)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    starts = starts[starts < n]
    run_of = np.zeros(n, dtype=np.int64)
    run_of[starts] = 1
    run_of[offs[:-1][offs[:-1] < n]] = 1
    run_of = np.cumsum(run_of) - 1
    types = TYPES[rng.integers(0, len(TYPES), size=int(run_of[-1]) + 1 if n else 0)]
    out["type"][flat] = types[run_of]
    ordinal = (rng.random(n) < 0.3).astype(np.uint32)
    out["aux"][flat] = (out["aux"][flat] & ~np.uint32(1)) | ordinal
    out["t"][flat] = out["t"][flat] + rng.uniform(-0.5, 0.5, size=n)
    return out


def alternating_drop_case(name, recs):
    """the types as drawn hold, on one curve, a run longer than 1 followed by at least three maximal runs of length 1"""
    offs, flat, _ = traced(name)
    ty = recs["type"][flat]
    for c in range(len(offs) - 1):
        t = ty[offs[c]:offs[c + 1]]
        if len(t) < 5:
            continue
        cut = np.flatnonzero(t[1:] != t[:-1]) + 1
        lens = np.diff(np.concatenate([[0], cut, [len(t)]]))
        for k in range(len(lens) - 3):
            if lens[k] > 1 and lens[k + 1] == 1 and lens[k + 2] == 1 and lens[k + 3] == 1:
                return True
    return False


def effects(name, recs, ts):
    """which effects of the post-processing the trajectories `ts` (host result) show on these records"""
    offs, flat, loop = traced(name)
    where = np.full(len(recs), -1, dtype=np.int64)          # record -> position in the flat point array
    where[flat] = np.arange(len(flat))
    curve_of = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    e = {"more_trajectories": len(ts) > len(offs) - 1, "fewer_points": len(ts.indices) < len(flat),
         "type_changed": bool(np.any(ts.type != recs["type"][ts.indices])), "t_changed": bool(np.any(ts.t != recs["t"][ts.indices])),
         "reversed": False, "rotated": False}
    pos = where[ts.indices]
    seen = set()
    for k in range(len(ts)):
        a, b = ts.offsets[k], ts.offsets[k + 1]
        c = int(ts.id[k])
        n = offs[c + 1] - offs[c]
        if b - a >= 2 and n >= 3 and (pos[a + 1] - pos[a]) % n == n - 1:
            e["reversed"] = True
        if c not in seen:                                   # the first piece of curve c: without a rotation it holds the curve's first point
            seen.add(c)
            if loop[c] and b > a and not np.any(pos[a:b] == offs[c]):
                e["rotated"] = True
        assert np.all(curve_of[pos[a:b]] == c)
    return e


def can_rotate(name):
    """rotate() needs a loop curve that holds two types between equal ends: three points at least.  The only loop curve that
    woven_31x37x32 traces has two, so no drawing of types can rotate it; singular_terraces has 1 203 loop curves of three points and more."""
    offs, _, loop = traced(name)
    return bool(np.any((np.diff(offs) >= 3) & (loop == 1)))


def shows_every_effect(name, run_length, recs, ts):
    e = effects(name, recs, ts)
    if not can_rotate(name):
        assert not e.pop("rotated")
    return all(e.values()) and (run_length != 1.3 or alternating_drop_case(name, recs))


def same_trajectories(a, b):
    """field for field; t bit for bit"""
    return (all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("offsets", "indices", "type", "loop", "id"))
            and np.array_equal(a.t.view(np.uint64), b.t.view(np.uint64)))
