"""ftkx::resident_sweep (include/ftkx_shim.hh) -- what the patched reference tracker holds (patches/ftk-xl-hip.patch) -- through its whole
life on the GPU: tests/shim/resident_run.cpp, linked with libftkx.so, runs the scripts of tests/shim_resident_cases.py on the first steps
of committed fixtures, and every sweep must return what the oracle computes for it.

The expectation of a step, scope by scope: oracle.sweep(..., tag_mode = TAG_WORK_INDEX) on V and J from oracle.gradient* / oracle.jacobian*
under factor = oracle.scaling_factor(min(running, resolution(V_t), resolution(V_t+1))), `running` threaded through the steps.  Compared
bit for bit, with no tolerance: tag, type, x, t, scalar, which records are ordinal and which interval, the timestep in the aux word, the
factor, and the running resolution handed back.  (That value is the exact sticky minimum once it is below 2^-8 and the value handed in
until then, as include/ftkx.h documents for ftkx_sweep_series: shim_resident_cases.expectation threads both.)

Scenarios: (a) the callers' cadence for scalar, vector, 3D and all-three-arrays-given input; (b) cadence, close(), open() with the same
options, cadence again -- the patched 2D tracker's reset() -- under a type filter, robust = 0, degrees, rectilinear and explicit coordinates:
both halves equal the oracle and each other byte for byte; (c) re-open on another lattice and dimension with other options; (d) options
changed on a live context; (e) clear() with two snapshots resident and the next push at t0 + n -- the 3D tracker's reset path --, pop
down to empty, a series from t = 1000; (f) contract errors, which throw on the host and leave the object usable.

Before close() forgot the cached options, every case of (b) failed in `_assert_scope` at the first ordinal sweep after the re-open: the
second context ran on the library's defaults (EXACT64 tags, no filter, robust).  degrees, rect and explicit2 failed at `tag`; saddles
returned 43 ordinal records where the oracle has 23, norobust_3d 110 where it has 131.  (a) and (c) to (f) passed."""
import os
import subprocess

import numpy as np
import pytest

import shim_resident_cases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    from ftk_amd import build
    build.build()
    lib = os.path.join(ROOT, "ftk_amd")
    return R.compile_runner(tmp_path_factory.mktemp("resident_gpu") / "resident_run", ["-L" + lib, "-lftkx", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype="<f8"), np.ascontiguousarray(b, dtype="<f8")
    return a.shape == b.shape and bool(np.all((a.view("<u8") == b.view("<u8")) | (np.isnan(a) & np.isnan(b))))


def _assert_scope(got, ref, ordinal, t, what):
    print(f"{what}: {len(got)} records, the oracle has {len(ref)}")
    assert len(got) == len(ref), (what, len(got), len(ref))
    got, ref = got[np.argsort(got["tag"], kind="stable")], ref[np.argsort(ref["tag"], kind="stable")]
    assert np.array_equal(got["tag"], ref["tag"]), (what, "tag")
    assert np.array_equal(got["type"], ref["type"]), (what, "type")
    for f in ("x", "t"):
        assert _same_bits(got[f], ref[f]), (what, f)
    assert _same_bits(got["scalar"][:, 0], ref["scalar"][:, 0]), (what, "scalar")
    # the ordinal / interval split: the vector a record came back in, its aux word and the oracle agree
    assert np.all((got["aux"] & 1) == int(ordinal)) and np.all(ref["ordinal"] == int(ordinal)), (what, "ordinal bit")
    assert np.all((got["aux"] >> 1) == t), (what, "timestep in the aux word")


def _assert_step(name, i, got, want):
    ev = want["event"]
    what = f"{name} sweep {i} (t = {ev['t']})"
    print(f"{what}: factor {got['factor']} / {want['factor']}, running {got['running_in']!r} -> {got['running_out']!r}, expected {want['running_out']!r} (exact minimum {want['running_exact']!r})")
    assert got["factor"] == want["factor"], (what, got["factor"], want["factor"])
    assert np.float64(got["running_out"]).tobytes() == np.float64(want["running_out"]).tobytes(), (what, got["running_out"], want["running_out"])
    _assert_scope(got["ordinal"], want["ordinal"], True, ev["t"], what + " ordinal")
    if ev["interval"]:
        _assert_scope(got["interval_records"], want["interval"], False, ev["t"], what + " interval")
    else:
        assert len(got["interval_records"]) == 0, what


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_resident_sweep_returns_oracle_records(case, exe, tmp_path, oracle):
    script = R.CASES[case](oracle)
    want = R.expectation(oracle, script)
    R.check_not_vacuous(oracle, script, want)
    sp, ap = script.write(str(tmp_path))
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe, sp, ap, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (case, r.stderr[-3000:])
    entries = R.read_entries(out)
    R.check_structure(script, entries)
    sweeps = [e for e in entries if e["kind"] == "sweep"]
    assert len(sweeps) == len(want) > 0
    for i, (got, w) in enumerate(zip(sweeps, want)):
        _assert_step(case, i, got, w)
    if case in R.RERUN_CASES:
        # (b) the run after close() / open() is the run before it, byte for byte: records in the order they came, aux words, factors, running
        half = script.half
        first, second = entries[:half], entries[half:]
        assert len(first) == len(second) and [e["raw"] for e in first] == [e["raw"] for e in second], (case, "the second run differs from the first")
