"""ftk_amd/csrc/series_verdict.hpp WITHOUT a GPU: tests/hostcheck/series_verdict.cpp as a program of its own (no Python in the process),
under -fsanitize=address,undefined where g++ has the runtimes.

The completion verdict over the full product: every subset of AMBIGUOUS, MASKS_INVALID, INF, OVERFLOW, TAIL_PENDING, HALO_FULL (with every
subset of EARLY, ONE, LATE_DECLINE, FIX_ORDER on top, which must change nothing) x by_host x dist x short_chain x a pass open behind x the
lists still the pass's own, against the rule written out a second time; what follows a re-queue; the named cases (HALO_FULL over
TAIL_PENDING and only for a slab pass, OVERFLOW alone sets "grow first", TAIL_PENDING on a pass that was not queued short).

The growth: each of the four counts at capacity and one over -- untouched, or exactly x + x/8 + 1024.

The tail policy, step by step through plans and completions: the short chain and who takes it, 8192 / 8193 list entries and the sixteen
plans sat out (split plans among them), late declines once / twice / interrupted, sixteen non-slab asks after a one-launch redo, the
thresholds of `sparse` from both sides, and that every way out without records, and abort, change the members they should and no others.

The reported path: 4, 5, 2, 1 over every status and split, and when the order block is filled."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "series_verdict.cpp")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_series_verdict(tmp_path):
    exe = str(tmp_path / "series_verdict")
    flags = ["-std=c++17", "-O1", "-g", "-Wall"]
    if _runtime("libasan.so") and _runtime("libubsan.so"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(["g++"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "series_verdict checks complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
