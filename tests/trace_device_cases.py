"""Record sets for tests/test_gpu_trace_device.py, built the same way by the test and by whoever checks its seeds on a CPU."""
import numpy as np

from common import load_golden

FIXTURES = ["woven_31x37x32", "woven_128x128x10", "double_gyre_64x32x50", "moving_extremum_3d_21x21x21x32", "merger_2d_32x32x100",
            "moving_extremum_3d_21x21x21x4_overflow", "singular_terraces_72x64x56x8"]

# Fragmented sets: every record of the fixture is kept with probability p.  Per (fixture, p) eight seeds; each of them, checked on the host
# path, leaves at least one lone point and at least one curve of two points with its loop flag set (the test asserts it again).  Seeds
# 0..7 wherever they do; a seed that does not was replaced by the next integer that does.
FRAGMENT_SEEDS = {
    ("woven_31x37x32", 0.9): [0, 1, 2, 3, 4, 5, 6, 7],
    ("woven_31x37x32", 0.5): [0, 1, 2, 3, 4, 5, 6, 7],
    ("woven_31x37x32", 0.15): [0, 1, 2, 3, 4, 5, 6, 7],
    ("moving_extremum_3d_21x21x21x4_overflow", 0.9): [0, 1, 2, 3, 4, 5, 6, 7],
    ("moving_extremum_3d_21x21x21x4_overflow", 0.5): [0, 1, 2, 3, 4, 5, 6, 7],
    ("moving_extremum_3d_21x21x21x4_overflow", 0.15): [0, 1, 2, 3, 4, 5, 6, 7],
}

_cache = {}


def fixture_records(name):
    """-> (golden dict, domain, records sorted by tag, with the aux word of the sweep); loaded once, never changed"""
    import ftk_amd
    if name not in _cache:
        g = load_golden(name)
        ref = g["records"]
        recs = np.zeros(len(ref), dtype=ftk_amd.CP_DTYPE)
        for f in ("tag", "type", "x", "t"):
            recs[f] = ref[f]
        recs["aux"] = (ref["ordinal"].astype(np.uint32) & 1) | (ref["timestep"].astype(np.uint32) << 1)
        recs = recs[np.argsort(recs["tag"], kind="stable")]
        recs.setflags(write=False)
        scalar = g["nv"] == 1
        lo = 2 if scalar else 1
        dom = ([lo] * g["nd"], [d - (3 if scalar else 2) for d in g["dims"]])
        _cache[name] = (g, dom, recs)
    return _cache[name]


def fragment(recs, p, seed):
    keep = np.random.default_rng([seed, int(round(p * 100))]).random(len(recs)) < p
    return recs[keep]


def has_lone_point_and_two_point_loop(curves, loop):
    lens = np.array([len(c) for c in curves])
    return bool(np.any(lens == 1)) and bool(np.any((lens == 2) & (np.asarray(loop) == 1)))
