"""Scripts for tests/shim/resident_run.cpp -- the whole life of ftkx::resident_sweep (include/ftkx_shim.hh): open, options, coordinates,
pushes, sweeps, pops, clear, close, re-open, contract errors -- with a model of what each script hands over, so that
tests/test_shim_resident_host.py (a recording stub in place of the library; no GPU) and tests/test_gpu_shim_resident.py (libftkx.so
against the oracle) run the same scripts.  The arrays are the first steps of committed fixtures."""
import functools
import os
import subprocess

import numpy as np

from common import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = float(np.finfo(np.float64).max)
TAG_WORK_INDEX = 0

# ftkx_options (include/ftkx.h), as the C compiler lays it out
OPT_DTYPE = np.dtype([("jacobian_symmetric", "<i4"), ("robust", "<i4"), ("use_type_filter", "<i4"), ("type_filter", "<u4"), ("compute_degrees", "<i4"),
                      ("tag_mode", "<i4"), ("exact_only", "<i4"), ("derive_jacobian", "<i4"), ("coords_mode", "<i4"), ("coords_bounds", "<f8", (6,))], align=True)
assert OPT_DTYPE.itemsize == 88
OPT_FIELDS = [n for n in OPT_DTYPE.names if n != "coords_bounds"]


@functools.lru_cache(maxsize=None)
def golden(name):
    return load_golden(name)


class Snapshot:
    """step k of a fixture as one of the three ways a snapshot reaches resident_sweep: 'scalar' (push_scalar: V and J derived on the device),
    'vector' (push with V alone: J derived) and 'all' (push with V, J and S given, derived here by the oracle from the scalar field)"""

    def __init__(self, name, k, how):
        self.name, self.k, self.how = name, k, how

    @property
    def key(self):
        return (self.name, self.k, self.how)

    def given(self, oracle):
        """the arrays handed to push, in the order V, J, S (None: not given)"""
        V, J, S = fields(oracle, self.name, self.k)
        return {"scalar": (None, None, S), "vector": (V, None, None), "all": (V, J, S)}[self.how]


_FIELDS = {}


def fields(oracle, name, k):
    """(V, J, S) of step k the way the reference derives them (critical_point_tracker_2d_regular.hh:238-261, 3d:125-148): computed once, shared"""
    if (name, k) not in _FIELDS:
        g = golden(name)
        a = np.ascontiguousarray(g["steps"][k], dtype=np.float64)
        if g["nv"] == 1:
            V = oracle.gradient2D(a) if g["nd"] == 2 else oracle.gradient3D(a)
            J = oracle.jacobian2D(V, True) if g["nd"] == 2 else oracle.jacobian3D(V)
            S = a
        else:
            V, S = a, None
            J = oracle.jacobian2D(V, False) if g["nd"] == 2 else oracle.jacobian3D(V)
        for x in (V, J, S):
            if x is not None:
                x.setflags(write=False)
        _FIELDS[(name, k)] = (V, J, S)
    return _FIELDS[(name, k)]


class Script:
    """builds the script and the arrays file, and keeps the model: `events` (what the program must write, in order) and `pushes`
    (the options in force at every push that reaches the library)"""

    def __init__(self, name, oracle):
        self.name, self.oracle = name, oracle
        self.lines, self.chunks, self.offsets, self.n = [], [], {}, 0
        self.events, self.pushes = [], []
        self.geom = self.opts = self.coords = None
        self.resident, self.fresh = [], True          # [(t, Snapshot)]; the next sweep starts from DBL_MAX
        self.is_open = False

    # ---- arrays ----
    def _array(self, key, a):
        if a is None:
            return "-"
        if key not in self.offsets:
            a = np.ascontiguousarray(a, dtype="<f8").ravel()
            self.offsets[key] = self.n
            self.chunks.append(a); self.n += a.size
        return str(self.offsets[key])

    # ---- commands ----
    def open(self, fixture):
        g = golden(fixture)
        nd, D = g["nd"], g["dims"]
        lo, size = (2, [d - 3 for d in D]) if g["nv"] == 1 else (1, [d - 2 for d in D])        # the domains of the reference's callers (json_interface.hh:640-653)
        self.geom = dict(nd=nd, dims=list(D), dom=([lo] * nd, size))
        v = [lo] * nd + size + [lo] * nd + size + list(D)
        self.lines.append(f"open {nd} 0 " + " ".join(str(x) for x in v))
        self.resident, self.coords, self.is_open = [], None, True
        return self

    def options(self, **o):
        assert set(o) <= set(OPT_FIELDS), o
        self.opts = dict(o)
        self.lines.append("options " + " ".join(f"{k}={int(v)}" for k, v in o.items()))
        return self

    def coordinates(self, fixture):
        g = golden(fixture)
        if g["rectilinear"] is not None:
            self.coords = ("rect", fixture)
            self.lines.append("rect " + " ".join(self._array((fixture, "rect", d), r) for d, r in enumerate(g["rectilinear"])))
        else:
            e = g["explicit"]                                                                   # (n1, n0, ncomp) = ndarray (ncomp, n0, n1)
            self.coords = ("explicit", fixture)
            self.lines.append(f"explicit {e.shape[2]} {e.shape[1]} {e.shape[0]} " + self._array((fixture, "explicit"), e))
        return self

    def push(self, t, snap, throws=False):
        V, J, S = snap.given(self.oracle)
        a = [self._array(snap.key + (w,), x) for w, x in (("V", V), ("J", J), ("S", S))]
        line = f"push_scalar {t} {a[2]}" if snap.how == "scalar" else f"push {t} {a[0]} {a[1]} {a[2]}"
        if throws:
            self.lines.append("expect_throw " + line)
            self.events.append(dict(kind="throw"))
            return self
        self.lines.append(line)
        self.pushes.append(dict(t=t, opts=dict(self.opts), coords=self.coords, how=snap.how, key=snap.key))
        self.resident.append((t, snap))
        return self

    def sweep(self, t, interval, throws=False):
        if throws:
            self.lines.append(f"expect_throw sweep {t} {int(interval)}")
            self.events.append(dict(kind="throw"))
            return self
        assert self.resident and self.resident[0][0] == t and len(self.resident) == (2 if interval else 1)
        self.lines.append(f"sweep {t} {int(interval)}")
        self.events.append(dict(kind="sweep", t=t, interval=bool(interval), snaps=[s for _, s in self.resident], geom=self.geom, opts=dict(self.opts),
                                coords=self.coords, fresh=self.fresh))
        self.fresh = False
        return self

    def _popped(self, popped):
        front = self.resident[0][0] if self.resident else None          # front_timestep() means something while size() > 0
        self.events.append(dict(kind="pop", popped=popped, size=len(self.resident), front=front, active=self.is_open))

    def pop(self):
        self.lines.append("pop")
        popped = bool(self.is_open and self.resident)
        if popped:
            self.resident.pop(0)
        self._popped(popped)
        return self

    def clear(self):
        self.lines.append("clear")
        self.resident = []
        self._popped(True)
        return self

    def close(self):
        self.lines.append("close")
        self.resident, self.is_open = [], False
        return self

    def fresh_running(self):
        self.lines.append("running max")
        self.fresh = True
        return self

    def cadence(self, fixture, ks, how, t0=0):
        """the loop of the tracker's callers: push t and t + 1, sweep(t, interval), pop, ..., a last ordinal sweep; one snapshot stays"""
        for i, k in enumerate(ks):
            self.push(t0 + i, Snapshot(fixture, k, how))
            if i:
                self.sweep(t0 + i - 1, True).pop()
        return self.sweep(t0 + len(ks) - 1, False)

    # ---- files ----
    def write(self, directory):
        os.makedirs(directory, exist_ok=True)
        script, arrays = os.path.join(directory, self.name + ".txt"), os.path.join(directory, self.name + ".f64")
        with open(script, "w") as f:
            f.write("\n".join(self.lines) + "\n")
        (np.concatenate(self.chunks) if self.chunks else np.zeros(0)).astype("<f8").tofile(arrays)
        return script, arrays


def options_of(fixture, how):
    """what the patched tracker hands over for this fixture (patches/ftk-xl-hip.patch: hip_push_snapshot), every field spelled out"""
    g = golden(fixture)
    mode = 2 if g["rectilinear"] is not None else 3 if g["explicit"] is not None else 0
    return dict(jacobian_symmetric=int(g["nv"] == 1), robust=int(g["robust"]), use_type_filter=int(bool(g["type_filter"])), type_filter=int(g["type_filter"] or 0),
                compute_degrees=int(g["degrees"]), derive_jacobian=int(how != "all"), coords_mode=mode)


def _start(name, oracle, fixture, how, **override):
    s = Script(name, oracle).open(fixture)
    g = golden(fixture)
    if g["rectilinear"] is not None or g["explicit"] is not None:
        s.coordinates(fixture)
    return s.options(**dict(options_of(fixture, how), **override))


# S2: the 2D scalar fixture; its type filter (saddles) is on only where a script says so
S2 = S2F = "random_2d_scalar_29x24x6_saddles"
V2, S3 = "random_2d_vector_23x20x5", "random_3d_scalar_13x12x11x4"
# robust = 0 in 3D: random_3d_scalar_13x12x11x4_norobust holds the records of the robust run (no simplex of it hangs on the robust test), so a
# library that ignored the flag would pass on it; the adversarial fixture has simplices that do
S3N = "adversarial_3d_scalar_9x9x9x3_norobust"
WOVEN, DEGREES, RECT, EXPLICIT2 = "woven_31x37x32", "woven_31x37x6_degrees", "random_2d_scalar_29x24x6_rect", "random_2d_scalar_29x24x6_explicit2"
NO_FILTER = dict(use_type_filter=0, type_filter=0)


def _cadence(name, fixture, ks, how, **override):
    return lambda oracle: _start(name, oracle, fixture, how, **override).cadence(fixture, ks, how)


def _rerun(name, fixture, ks, how, **override):
    """(b) cadence, close, open on the same lattice with the same options, cadence again from a fresh running resolution: what the patched
    2D tracker's reset() makes of the object (hip_reset -> close(); the next push opens a new context and hands the same options over)"""
    def make(oracle):
        s = _start(name, oracle, fixture, how, **override).cadence(fixture, ks, how)
        s.half = len(s.events)
        s.close().fresh_running()
        g = golden(fixture)
        s.open(fixture)
        if g["rectilinear"] is not None or g["explicit"] is not None:
            s.coordinates(fixture)
        return s.options(**dict(options_of(fixture, how), **override)).cadence(fixture, ks, how)
    return make


def _pops_on_nothing(oracle):
    """pop and clear on an object that is not open, on an open one that holds nothing, and after close(): no drop reaches the library"""
    s = Script("host_pops_on_nothing", oracle)
    s.pop().clear()
    s.open(S2).options(**options_of(S2, "scalar")).pop().clear().pop()
    s.push(4, Snapshot(S2, 0, "scalar")).push(5, Snapshot(S2, 1, "scalar")).pop().pop().pop().clear()
    s.push(7, Snapshot(S2, 2, "scalar")).close().pop().clear()
    return s


def _reopen(oracle):
    """(c) one object on three lattices, 31 x 37 -> 29 x 24 -> 9 x 9 x 9, with other options every time; open() closes what was open"""
    s = _start("c_reopen_other_lattice", oracle, DEGREES, "scalar").cadence(DEGREES, range(3), "scalar")
    s.fresh_running().open(S2F).options(**options_of(S2F, "scalar")).cadence(S2F, range(3), "scalar", t0=5)
    s.close().fresh_running().open(S3N).options(**options_of(S3N, "scalar")).cadence(S3N, range(3), "scalar")
    return s


def _live_options(oracle):
    """(d) the type filter goes on after step 1 and off after step 3, on a live context"""
    s = _start("d_options_on_live_context", oracle, S2, "scalar", **NO_FILTER)
    on, off = options_of(S2F, "scalar"), dict(options_of(S2F, "scalar"), **NO_FILTER)
    s.push(0, Snapshot(S2, 0, "scalar"))
    for t in range(1, 6):
        s.push(t, Snapshot(S2, t, "scalar")).sweep(t - 1, True).pop()
        if t - 1 == 1:
            s.options(**on)
        if t - 1 == 3:
            s.options(**off)
    return s.sweep(5, False)


def _clear_3d(oracle):
    """(e) the 3D tracker's reset: clear() with two snapshots resident, the next push at t0 + n; then pop down to empty and push later still"""
    s = _start("e_clear_and_go_on_3d", oracle, S3, "scalar")
    s.push(0, Snapshot(S3, 0, "scalar")).push(1, Snapshot(S3, 1, "scalar")).sweep(0, True)
    s.clear().pop()                                                                 # (the pop finds nothing: no drop)
    s.push(2, Snapshot(S3, 2, "scalar")).push(3, Snapshot(S3, 3, "scalar")).sweep(2, True).pop().sweep(3, False)
    s.pop().pop().clear()                                                           # empty after the first pop
    return s.cadence(S3, [1, 0, 3], "scalar", t0=9)


def _late_start(oracle):
    return _start("e_series_from_t1000_3d", oracle, S3, "scalar").cadence(S3, range(4), "scalar", t0=1000)


def _contract_errors(oracle):
    """(f) each must throw and leave the object usable: host-side checks, nothing reaches the library"""
    s = Script("f_contract_errors", oracle)
    s.push(0, Snapshot(S2, 0, "scalar"), throws=True)                               # a push before open()
    s.open(S2).options(**dict(options_of(S2, "scalar"), **NO_FILTER))
    s.sweep(0, False, throws=True)                                                  # nothing resident
    s.push(0, Snapshot(S2, 0, "scalar"))
    s.sweep(1, False, throws=True)                                                  # the wrong t
    s.sweep(0, True, throws=True)                                                   # an interval sweep with one snapshot
    s.push(2, Snapshot(S2, 2, "scalar"), throws=True)                               # out of order
    s.push(0, Snapshot(S2, 0, "scalar"), throws=True)
    for t in range(1, 4):
        s.push(t, Snapshot(S2, t, "scalar"))
        s.sweep(t, True, throws=True)                                               # the wrong t with two resident
        s.sweep(t - 1, True).pop()
    return s.sweep(3, False)


CASES = {
    "a_cadence_2d_scalar": _cadence("a_cadence_2d_scalar", S2, range(6), "scalar", **NO_FILTER),
    "a_cadence_2d_vector": _cadence("a_cadence_2d_vector", V2, range(5), "vector"),
    "a_cadence_3d_scalar": _cadence("a_cadence_3d_scalar", S3, range(4), "scalar"),
    "a_cadence_all_given": _cadence("a_cadence_all_given", WOVEN, range(5), "all"),
    "b_rerun_saddles": _rerun("b_rerun_saddles", S2F, range(4), "scalar"),
    "b_rerun_norobust_3d": _rerun("b_rerun_norobust_3d", S3N, range(3), "scalar"),
    "b_rerun_degrees": _rerun("b_rerun_degrees", DEGREES, range(4), "scalar"),
    "b_rerun_rect": _rerun("b_rerun_rect", RECT, range(3), "scalar"),
    "b_rerun_explicit2": _rerun("b_rerun_explicit2", EXPLICIT2, range(3), "scalar"),
    "c_reopen_other_lattice": _reopen,
    "d_options_on_live_context": _live_options,
    "e_clear_and_go_on_3d": _clear_3d,
    "e_series_from_t1000_3d": _late_start,
    "f_contract_errors": _contract_errors,
}
RERUN_CASES = [n for n in CASES if n.startswith("b_")]
# for the recording stub alone (no sweep result to compare): a non-default type filter together with robust = 0 across close / open, and
# pop / clear where there is nothing to drop
HOST_CASES = {
    "host_rerun_filter_and_norobust": _rerun("host_rerun_filter_and_norobust", S2F, range(3), "scalar", robust=0, type_filter=6),
    "host_pops_on_nothing": _pops_on_nothing,
}


# ---- the program and what it writes ----
CP_DTYPE = np.dtype([("x", "<f8", (3,)), ("t", "<f8"), ("scalar", "<f8", (3,)), ("type", "<u4"), ("aux", "<u4"), ("tag", "<u8")])
assert CP_DTYPE.itemsize == 72


def compile_runner(exe, against, flags=()):
    """resident_run.cpp with `against`: the link arguments of the library under it"""
    cmd = ["g++", "-std=c++17", "-O1", "-g", *flags, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim", "resident_run.cpp"), "-o", str(exe), *against]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def read_entries(path):
    """-> list of dicts, one per entry of the program's output; 'raw' = the entry's bytes"""
    raw = open(path, "rb").read()
    off, out = 0, []
    while off < len(raw):
        start = off
        kind = int(np.frombuffer(raw, "<u4", 1, off)[0]); off += 4
        if kind == 1:
            t, interval = (int(v) for v in np.frombuffer(raw, "<i4", 2, off)); off += 8
            rin, rout = (float(v) for v in np.frombuffer(raw, "<f8", 2, off)); off += 16
            factor, no, ni = (int(v) for v in np.frombuffer(raw, "<u8", 3, off)); off += 24
            ordinal = np.frombuffer(raw, CP_DTYPE, no, off).copy(); off += 72 * no
            between = np.frombuffer(raw, CP_DTYPE, ni, off).copy(); off += 72 * ni
            out.append(dict(kind="sweep", t=t, interval=bool(interval), running_in=rin, running_out=rout, factor=factor, ordinal=ordinal, interval_records=between))
        elif kind == 2:
            out.append(dict(kind="throw", thrown=bool(np.frombuffer(raw, "<u4", 1, off)[0]))); off += 4
        elif kind == 3:
            popped = bool(np.frombuffer(raw, "<u4", 1, off)[0]); off += 4
            size = int(np.frombuffer(raw, "<u8", 1, off)[0]); off += 8
            front = int(np.frombuffer(raw, "<i4", 1, off)[0]); off += 4
            active = bool(np.frombuffer(raw, "<u4", 1, off)[0]); off += 4
            out.append(dict(kind="pop", popped=popped, size=size, front=front, active=active))
        else:
            raise AssertionError(f"{path}: entry kind {kind} at byte {start}")
        out[-1]["raw"] = raw[start:off]
    return out


def check_structure(script, entries):
    """what does not depend on the library: the entries are the script's, every expect_throw threw, pop / clear report the model's deque"""
    assert [e["kind"] for e in entries] == [e["kind"] for e in script.events], (script.name, [e["kind"] for e in entries])
    for i, (got, want) in enumerate(zip(entries, script.events)):
        if want["kind"] == "throw":
            assert got["thrown"], (script.name, i, "no std::runtime_error")
        elif want["kind"] == "pop":
            assert (got["popped"], got["size"], got["active"]) == (want["popped"], want["size"], want["active"]), (script.name, i, got, want)
            if want["front"] is not None:
                assert got["front"] == want["front"], (script.name, i, got, want)
        else:
            assert (got["t"], got["interval"]) == (want["t"], want["interval"]), (script.name, i)
            assert got["running_in"] == (DBL_MAX if want["fresh"] else entries_running_before(entries, i)), (script.name, i, got["running_in"])


def entries_running_before(entries, i):
    for e in reversed(entries[:i]):
        if e["kind"] == "sweep":
            return e["running_out"]
    return DBL_MAX


# ---- what the oracle says every sweep of a script returns ----
_SWEEPS = {}


def oracle_sweep(oracle, ev, scope, factor, tag_mode=TAG_WORK_INDEX, **override):
    """oracle.sweep of one scope of one step of a script, under the script's options at that step (override: other options); computed once"""
    o = dict(ev["opts"], **override)
    key = (tuple(s.key for s in ev["snaps"]), ev["t"], scope, int(factor), tag_mode, tuple(sorted(o.items())), ev["coords"], tuple(ev["geom"]["dims"]))
    if key not in _SWEEPS:
        g = ev["geom"]
        F = [fields(oracle, s.name, s.k) for s in ev["snaps"]] + [(None, None, None)]
        pair = lambda i: (F[0][i], F[1][i])                                           # noqa: E731
        coords = {}
        if ev["coords"] is not None:
            kind, fixture = ev["coords"]
            coords = dict(rectilinear=golden(fixture)["rectilinear"]) if kind == "rect" else dict(explicit=golden(fixture)["explicit"])
        r = oracle.sweep(g["nd"], scope, ev["t"], g["dom"], g["dom"], ([0] * g["nd"], g["dims"]), pair(0), pair(1), None if F[0][2] is None else pair(2), factor,
                         jacobian_symmetric=bool(o.get("jacobian_symmetric", 0)), robust=bool(o.get("robust", 0)),
                         type_filter=int(o["type_filter"]) if o.get("use_type_filter") else None, compute_degrees=bool(o.get("compute_degrees", 0)),
                         tag_mode=tag_mode, **coords)
        r.setflags(write=False)
        _SWEEPS[key] = r
    return _SWEEPS[key]


def expectation(oracle, script):
    """for every sweep of the script, in order: dict(factor, running_exact, running_out, ordinal, interval (None: not swept)).
    factor = scaling_factor(min(running, resolution(V_t), resolution(V_t+1))) with the EXACT sticky minimum (critical_point_tracker.hh:850-864).
    running_out is what sweep() hands back for the running resolution it was given, as include/ftkx.h documents it for ftkx_sweep_series: the
    minimum counts a slice's resolution only where it is below 1 / hint, hint = max(scaling_factor(running in), 256) -- a value at or above
    that cannot change the factor -- so it is the exact minimum once that is below 2^-8 and the value handed in (DBL_MAX at first) until
    then.  Both are threaded through the steps; they always give the same factor (asserted)."""
    out, exact, handed = [], DBL_MAX, DBL_MAX
    for ev in script.events:
        if ev["kind"] != "sweep":
            continue
        if ev["fresh"]:
            exact = handed = DBL_MAX
        res = [oracle.resolution(fields(oracle, s.name, s.k)[0]) for s in ev["snaps"]]
        exact = min([exact] + res)
        factor = oracle.scaling_factor(exact)[0]
        hint = max(oracle.scaling_factor(handed)[0], 256)
        handed = min([handed] + [r for r in res if r < 1.0 / hint])
        assert oracle.scaling_factor(handed)[0] == factor, (script.name, ev["t"], handed, exact)
        out.append(dict(factor=factor, running_exact=exact, running_out=handed, ordinal=oracle_sweep(oracle, ev, 1, factor),
                        interval=oracle_sweep(oracle, ev, 2, factor) if ev["interval"] else None, event=ev))
    return out


def _differs(a, b):
    return len(a) != len(b) or not np.array_equal(np.sort(a["tag"]), np.sort(b["tag"])) or a["type"][np.argsort(a["tag"], kind="stable")].tobytes() != b["type"][np.argsort(b["tag"], kind="stable")].tobytes()


def check_not_vacuous(oracle, script, want):
    """the conditions under which a wrong library could still pass, ruled out on the oracle alone: every sweep finds records in every scope it
    sweeps; under the type filter, and in 3D with robust = 0, the option changes the oracle's records of every sweep; and the tags the
    library's DEFAULT tag mode (EXACT64) would give differ from the work indices, so a context left on its defaults cannot pass"""
    seen = dict(filter=[], robust=[], tags=[])
    for w in want:
        ev = w["event"]
        for scope, recs in ((1, w["ordinal"]), (2, w["interval"])):
            if recs is None:
                continue
            assert len(recs) > 0, (script.name, ev["t"], scope, "the oracle finds nothing here")
            if ev["opts"].get("use_type_filter"):
                seen["filter"].append(_differs(recs, oracle_sweep(oracle, ev, scope, w["factor"], use_type_filter=0, type_filter=0)))
            if ev["geom"]["nd"] == 3 and not ev["opts"].get("robust"):
                seen["robust"].append(_differs(recs, oracle_sweep(oracle, ev, scope, w["factor"], robust=1)))
            seen["tags"].append(not np.array_equal(np.sort(recs["tag"]), np.sort(oracle_sweep(oracle, ev, scope, w["factor"], tag_mode=2)["tag"])))
    assert all(seen["tags"]), (script.name, "EXACT64 tags equal the work indices somewhere")
    assert all(seen["filter"]), (script.name, "the type filter changes nothing somewhere", seen["filter"])
    assert all(seen["robust"]), (script.name, "robust = 0 changes nothing somewhere", seen["robust"])
    return seen
