"""ftk_amd/csrc/ctx_block.hpp WITHOUT a GPU: tests/hostcheck/ctx_block.cpp as a program of its own (no Python in the process), under
-fsanitize=address,undefined (leak detection on) where g++ has the runtimes.  The program defines the three raw functions behind
ftkx_block over malloc and free, counts their calls and checks: a reserve at or below `bytes` does nothing; a growing one drains (only
with a stream, only when the block held memory), then frees once, then allocates `alloc` bytes and reports fresh memory; a failed
allocation leaves the block empty with the out-of-memory status and the next reserve succeeds; moving empties the source; an owning
block is freed exactly once; and the patch staging that was admitted by cells (4 >= 4) and overran grows when admitted by bytes.
The lent kind: never passed to ftkx_block_free, a move empties the source, reserve is an error, the pool lets it go.  The pool of the
slice arrays (ftkx_array_pool): a take after a give of the same class and bytes returns the same memory; never another class's, never for
more or fewer bytes; newest first; the cap frees the surplus once; clear frees all; a failed allocation leaves nothing behind; and an array
of the old lattice that comes back after the pool was cleared for a larger one is not handed out for the larger one."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "ctx_block.cpp")


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_block(tmp_path):
    exe = str(tmp_path / "ctx_block")
    flags = ["-std=c++17", "-O1", "-g", "-Wall"]
    if _runtime("libasan.so") and _runtime("libubsan.so"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(["g++"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ctx_block checks complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
