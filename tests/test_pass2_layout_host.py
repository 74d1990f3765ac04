"""ftk_amd/csrc/pass2_layout.hpp WITHOUT a GPU: tests/hostcheck/pass2_layout.cpp as a program of its own (no Python in the process),
under -fsanitize=address,undefined where g++ has the runtimes.  For maxnb in {6, 8} and n in {1, 2, 5, 100, 150, 4096, 4097} it checks
that every array of the trace's, the ordering's and the post-processing's layout lies inside its total, overlaps no other and starts on
its element's alignment, that the shared prefixes agree on both sides, that nbr .. deg is one range, and -- for every ordered pair of
cases -- that a block reserved for the first holds every array of the second, the union-find's parents included, whenever the second's
total lets it in."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "pass2_layout.cpp")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_layouts(tmp_path):
    exe = str(tmp_path / "pass2_layout")
    flags = ["-std=c++17", "-O1", "-g", "-Wall"]
    if _runtime("libasan.so") and _runtime("libubsan.so"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(["g++"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "pass2_layout checks complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
