"""ftk_amd/csrc/series_order.hpp WITHOUT a GPU: tests/hostcheck/series_order.cpp as a program of its own (no Python in the process),
under -fsanitize=address,undefined where g++ has the runtimes.

The repair of the buckets the rank kernel leaves to the host (SERIES_FIX_ORDER) against std::sort: every permutation of up to 8 tags,
20 000 random concatenations of runs that are each in order or shuffled (every tag of a run below every tag of the next, with and
without repeated tags), a fat run first, last, two side by side, alone and between thin ones, n = 0 and 1; the records keep their other
members and nothing outside them is written.

The bucket geometry for n * cells * 64 around every power of two up to 2^50 and bins of 0, 1, 10, 14, 16 (and -3, 17, 40: clamped):
((max_key - 1) >> shift) + 1 == nbins <= 2^16, no more buckets than asked for and more than half as many wherever shift > 0, every key
below max_key in a bucket below nbins."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "series_order.cpp")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_series_order(tmp_path):
    exe = str(tmp_path / "series_order")
    flags = ["-std=c++17", "-O1", "-g", "-Wall"]
    if _runtime("libasan.so") and _runtime("libubsan.so"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(["g++"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "series_order checks complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
