"""ftkx::resident_sweep (include/ftkx_shim.hh) on its own, without a GPU: tests/shim/resident_run.cpp runs every script of
tests/shim_resident_cases.py -- cadence, close and re-open, another lattice, options changed on a live context, clear / pop down to
empty, contract errors -- linked with tests/shim/ftkx_stub.cpp, which records every call into the C ABI.  What the object must have
handed to the library is read from that record, call by call:
  * every context that receives a snapshot received ftkx_set_options first, with tag_mode == FTKX_TAG_WORK_INDEX (what from_work_index()
    at the reference's call sites decodes) and the options most recently given -- also the context opened after close();
  * the coordinates of a re-opened context are sent again; every snapshot is the array the script named, at the script's timestep;
  * no ftkx_drop_slice beyond what is resident, and no call that the library would refuse;
  * equal options given again on a live context are not sent again.
The same program is built once more with -fsanitize=address,undefined (a stand-alone program: nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

import shim_resident_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "shim", "ftkx_stub.cpp")
ALL_CASES = dict(R.CASES, **R.HOST_CASES)
PUSHES = ("ftkx_push_slice", "ftkx_push_scalar_slice")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    return R.compile_runner(tmp_path_factory.mktemp("resident_stub") / "resident_run_stub", [STUB])


def run_on_stub(exe, script, tmp, env=None):
    """-> (the program's entries, the stub's record as a list of (entry point, {name: value}))"""
    sp, ap = script.write(str(tmp))
    out, log = os.path.join(str(tmp), script.name + ".out"), os.path.join(str(tmp), script.name + ".log")
    r = subprocess.run([exe, sp, ap, out], capture_output=True, text=True, timeout=300, env=dict(os.environ, FTKX_STUB_LOG=log, **(env or {})))
    assert r.returncode == 0, (script.name, r.stderr[-3000:])
    calls = []
    for line in open(log):
        name, *kv = line.split()
        calls.append((name, dict(x.split("=", 1) for x in kv)))
    return R.read_entries(out), calls, r.stderr


def _bytes(a):
    return None if a is None else np.ascontiguousarray(a, dtype="<f8").tobytes()


def _arg(v):
    return None if v == "null" else bytes.fromhex(v)


def check_calls(script, calls, oracle):
    assert all(kv["rc"] == "0" for _, kv in calls), [c for c in calls if c[1]["rc"] != "0"]          # nothing the library would refuse
    options, mesh, coords, resident, alive = {}, {}, {}, {}, set()
    pushes = iter(script.pushes)
    n_pushes = 0
    for i, (name, kv) in enumerate(calls):
        ctx = int(kv["ctx"])
        if name == "ftkx_create":
            assert ctx not in resident
            alive.add(ctx); resident[ctx] = []
            continue
        assert ctx in alive, (script.name, i, name, "a call on a context that was destroyed or never created")
        if name == "ftkx_destroy":
            alive.discard(ctx)
        elif name == "ftkx_set_mesh":
            mesh[ctx] = kv
        elif name == "ftkx_set_options":
            o = np.frombuffer(_arg(kv["opt"]), dtype=R.OPT_DTYPE)[0]
            assert ctx not in options or o.tobytes() != options[ctx].tobytes(), (script.name, i, "equal options sent twice to one live context")
            options[ctx] = o
        elif name in ("ftkx_set_coords_rectilinear", "ftkx_set_coords_explicit"):
            assert not resident[ctx], (script.name, i, "coordinates are fixed before the first snapshot")
            coords[ctx] = (name, kv)
        elif name in PUSHES:
            want = next(pushes, None)
            n_pushes += 1
            assert want is not None, (script.name, i, "more pushes than the script has")
            assert ctx in mesh, (script.name, i, "a snapshot for a context without a mesh")
            # THE property: this context -- not an earlier one at the same address -- was given the options, and they are the latest
            assert ctx in options, (script.name, i, f"context {ctx} receives snapshot t = {kv['t']} but never received ftkx_set_options: it runs on the library's defaults")
            o = options[ctx]
            assert int(o["tag_mode"]) == R.TAG_WORK_INDEX, (script.name, i, int(o["tag_mode"]))
            for f in R.OPT_FIELDS:
                if f != "tag_mode":
                    assert int(o[f]) == int(want["opts"].get(f, 0)), (script.name, i, f, int(o[f]), want["opts"])
            assert not o["coords_bounds"].any()
            # the snapshot itself
            assert int(kv["t"]) == want["t"] and kv["on_device"] == "0"
            assert name == ("ftkx_push_scalar_slice" if want["how"] == "scalar" else "ftkx_push_slice")
            V, J, S = R.Snapshot(*want["key"]).given(oracle)
            assert (_arg(kv["V"]), _arg(kv["J"]), _arg(kv["S"])) == (_bytes(V), _bytes(J), _bytes(S)), (script.name, i, "another array than the script named")
            # the coordinates of THIS context
            if want["coords"] is None:
                assert ctx not in coords
            else:
                kind, fixture = want["coords"]
                g = R.golden(fixture)
                assert ctx in coords, (script.name, i, "the re-opened context has no coordinates")
                cname, ckv = coords[ctx]
                if kind == "rect":
                    assert cname == "ftkx_set_coords_rectilinear"
                    assert [_arg(ckv[a]) for a in "xy"] == [_bytes(r) for r in g["rectilinear"][:2]] and (_arg(ckv["z"]) or b"") == b""
                else:
                    e = g["explicit"]
                    assert cname == "ftkx_set_coords_explicit" and (int(ckv["ncomp"]), int(ckv["n0"]), int(ckv["n1"])) == (e.shape[2], e.shape[1], e.shape[0])
                    assert _arg(ckv["coords"]) == _bytes(e)
            assert int(kv["t"]) == (resident[ctx][-1] + 1 if resident[ctx] else int(kv["t"])), (script.name, i, "not in timestep order")
            resident[ctx].append(int(kv["t"]))
        elif name == "ftkx_drop_slice":
            assert resident[ctx] and resident[ctx][0] == int(kv["t"]), (script.name, i, "a drop beyond what is resident", kv["t"], resident[ctx])
            resident[ctx].pop(0)
        elif name == "ftkx_sweep_series":
            ts = np.frombuffer(_arg(kv["timesteps"]), "<i4"); sc = np.frombuffer(_arg(kv["scopes"]), "<i4")
            assert len(ts) == 1 and resident[ctx] and resident[ctx][0] == ts[0] and len(resident[ctx]) >= (2 if sc[0] == 3 else 1) and sc[0] in (1, 3)
        else:
            raise AssertionError(f"{script.name}: unexpected entry point {name}")
    assert n_pushes == len(script.pushes), (script.name, n_pushes, len(script.pushes))
    assert not alive, (script.name, "contexts left alive at exit", alive)
    sweeps = [kv for name, kv in calls if name == "ftkx_sweep_series"]
    assert len(sweeps) == sum(e["kind"] == "sweep" for e in script.events)          # (a sweep that must throw never reaches the library)


@pytest.mark.parametrize("case", sorted(ALL_CASES))
def test_resident_sweep_hands_every_context_its_options(case, stub_exe, tmp_path, oracle):
    script = ALL_CASES[case](oracle)
    entries, calls, _ = run_on_stub(stub_exe, script, tmp_path)
    R.check_structure(script, entries)
    check_calls(script, calls, oracle)


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_scenarios_are_not_vacuous_on_the_oracle(case, oracle):
    """what tests/test_gpu_shim_resident.py compares with, computed here: every sweep of every script finds records in each scope it sweeps,
    the type filter and robust = 0 change the oracle's records where a script sets them, and the EXACT64 tags of the library's defaults
    differ from the work indices -- so a context left on its defaults, or a flag that did not arrive, cannot pass there"""
    script = R.CASES[case](oracle)
    want = R.expectation(oracle, script)
    assert len(want) == sum(e["kind"] == "sweep" for e in script.events) > 0
    seen = R.check_not_vacuous(oracle, script, want)
    if any(w["event"]["opts"].get("use_type_filter") for w in want):
        assert seen["filter"]
    if "norobust" in case:
        assert seen["robust"]


def test_reopened_context_carries_type_filter_and_robust_off(stub_exe, tmp_path, oracle):
    """close() and open() with the same options: the struct forwarded to the SECOND context carries the type filter and robust = 0"""
    script = R.HOST_CASES["host_rerun_filter_and_norobust"](oracle)
    _, calls, _ = run_on_stub(stub_exe, script, tmp_path)
    created = [int(kv["ctx"]) for name, kv in calls if name == "ftkx_create"]
    assert len(created) == 2 and created[0] != created[1]
    sent = {c: [np.frombuffer(_arg(kv["opt"]), dtype=R.OPT_DTYPE)[0] for name, kv in calls if name == "ftkx_set_options" and int(kv["ctx"]) == c] for c in created}
    assert len(sent[created[0]]) == 1, "equal options on one live context are forwarded once"
    assert len(sent[created[1]]) == 1, "the context opened after close() was never given the options"
    o = sent[created[1]][0]
    assert (int(o["use_type_filter"]), int(o["type_filter"]), int(o["robust"]), int(o["tag_mode"])) == (1, 6, 0, R.TAG_WORK_INDEX)
    assert o.tobytes() == sent[created[0]][0].tobytes()


@pytest.mark.skipif(_runtime("libasan.so") is None or _runtime("libubsan.so") is None, reason="sanitizer runtimes not installed")
def test_resident_sweep_is_clean_under_asan_ubsan(tmp_path, oracle):
    exe = R.compile_runner(tmp_path / "resident_run_stub_san", [STUB], flags=["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for case in sorted(ALL_CASES):
        script = ALL_CASES[case](oracle)
        entries, calls, err = run_on_stub(exe, script, tmp_path, env=env)
        assert "Sanitizer" not in err and "runtime error" not in err, (case, err[-3000:])
        R.check_structure(script, entries)
        check_calls(script, calls, oracle)
