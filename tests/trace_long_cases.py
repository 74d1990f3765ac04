"""Record sets with ONE very long chain for tests/test_gpu_trace_long_chains.py: the device trace ranks the records of a curve by pointer
jumping, and the fixtures' curves are done after 1-4 launches of it.  Here a path and a cycle of more than 20 000 records each, and the
path cut into pieces of chosen lengths.  The records come from the CPU oracle's sweep (oracle/pyoracle.py; the parity tests hold the GPU
sweep to it bit for bit) of two scalar series on a 24 x 16 grid, so everything a set has to show is asserted without a GPU
(tests/test_trace_long_cases.py).  Timesteps stay far below 2^24, the room the device trace's order key has for them.

  open     synthetic.moving_extremum with dyadic parameters: a minimum that starts at (3.25, 3.375) and moves by (1/512, 1/1024) per
           step, 7 000 steps: it ends at (16.92, 10.21), inside the domain.  One path, three records per step.
  closed   S = (x - x0)^3 / 3 - a(t) (x - x0) + (y - y0)^2 with x0 = 12.3125, y0 = 8.40625 (off the vertices) and a(t) a parabola
           in t: negative during the first and last 40 of 3 600 steps, 36 at its top.  The central-difference gradient vanishes at
           x = x0 +- sqrt(a - 1/3), y = y0: a saddle and a minimum are born together, move apart by up to 6 cells and die together -- one
           closed curve through both.
  cut      the open path without nine of its records, chosen along the host's curve so that the pieces have 1, 2, 3, 16, 17, 256, 257,
           4 096 and 4 097 points, and one more what is left."""
import numpy as np

DW, DH = 24, 16
DOMAIN = ([2, 2], [DW - 3, DH - 3])
OPEN_STEPS, CLOSED_STEPS, CLOSED_LEAD, CLOSED_TOP = 7000, 3600, 40, 36.0
OPEN_X0, OPEN_V = (3.25, 3.375), (1.0 / 512, 1.0 / 1024)
CLOSED_X0 = (12.3125, 8.40625)
MIN_POINTS = 20000
PIECES = [1, 2, 3, 16, 17, 256, 257, 4096, 4097]

_cache = {}


def open_field(k):
    from ftk_amd import synthetic
    import torch
    return synthetic.moving_extremum((DW, DH), k, OPEN_X0, OPEN_V, torch, "cpu").numpy()


def closed_field(k):
    x = np.arange(DW, dtype=np.float64)[None, :] - CLOSED_X0[0]
    y = np.arange(DH, dtype=np.float64)[:, None] - CLOSED_X0[1]
    s = (k - CLOSED_LEAD) / float(CLOSED_STEPS - 1 - 2 * CLOSED_LEAD)
    a = CLOSED_TOP * 4.0 * s * (1.0 - s)
    return x ** 3 / 3.0 - a * x + y ** 2


def _sweep(field, nsteps):
    import ftk_amd
    import pyoracle
    ref, _, _ = pyoracle.track([field(k) for k in range(nsteps)], 2, 1, tag_mode=pyoracle.TAG_EXACT64, nthreads=1)
    recs = np.zeros(len(ref), dtype=ftk_amd.CP_DTYPE)
    for f in ("tag", "type", "x", "t"):
        recs[f] = ref[f]
    recs["aux"] = (ref["ordinal"].astype(np.uint32) & 1) | (ref["timestep"].astype(np.uint32) << 1)
    return recs[np.argsort(recs["tag"], kind="stable")]


def records(name):
    """-> records sorted by tag, with the aux word of the sweep; made once per process, never changed"""
    import ftk_amd
    if name not in _cache:
        if name == "open":
            recs = _sweep(open_field, OPEN_STEPS)
        elif name == "closed":
            recs = _sweep(closed_field, CLOSED_STEPS)
        elif name == "cut":
            full = records("open")
            curves, _, _ = ftk_amd.trace_curves(2, DOMAIN, full)
            assert len(curves) == 1
            at = np.cumsum(np.array(PIECES) + 1) - 1         # along the curve: a piece, a record taken out, the next piece, ...
            keep = np.ones(len(full), dtype=bool)
            keep[curves[0][at]] = False
            recs = full[keep]
        else:
            raise ValueError(name)
        recs.setflags(write=False)
        _cache[name] = recs
    return _cache[name]


def host_curves(name):
    """-> ftk_amd.trace_curves on the host; once per process"""
    import ftk_amd
    if ("host", name) not in _cache:
        _cache[("host", name)] = ftk_amd.trace_curves(2, DOMAIN, records(name))
    return _cache[("host", name)]


def shows_what_it_must(name):
    curves, loop, nspecial = host_curves(name)
    lens = sorted(len(c) for c in curves)
    n = len(records(name))
    if name == "open":
        return len(curves) == 1 and lens[0] >= MIN_POINTS and lens[0] == n and int(loop[0]) == 0 and nspecial == 0
    if name == "closed":
        return len(curves) == 1 and lens[0] >= MIN_POINTS and lens[0] == n and int(loop[0]) == 1 and nspecial == 0
    rest = len(records("open")) - sum(PIECES) - len(PIECES)
    return lens == sorted(PIECES + [rest]) and rest > 4097 and nspecial == 0
