#!/usr/bin/env python3
"""Pass 2's second half, A against B in one process, on the record sets of C2 (woven 1024^2 x 64) and C5 (double_gyre 2048 x 1024 x 128)
as the library's own sweep delivers them:

    post-processing   ftkx_post_process_curves (host threads)  against  ftkx_post_process_curves_device (maps and scans on the GPU),
                      both on the curves ftkx_trace_curves_device returned
    pass 2            ftkx_trace_curves_device + ftkx_post_process_curves  against  ftkx_pass2_device (the curves stay on the device)

    python tools/post_process_ab.py                 # every step as a child process under its own `timeout -k 10`, chained with &&
    python tools/post_process_ab.py --case C2       # one step: 5 warm-up calls of each, then 30 calls each, interleaved A B A B ...
    python tools/post_process_ab.py --case C2 --phases   # the device forms' phases (FTKX_POST_PROCESS_PHASES, FTKX_TRACE_PHASES: the host waits after each)

Times are host clocks around the C calls, which end in a stream synchronise and return the finished trajectories.  Printed: the median and
the quartiles of each, the path each took, and whether the trajectories are identical in EVERY call (exit status 1 if not)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pass2_ab import CASES, records_of  # noqa: E402


def one_case(case, phases, calls, warmup):
    import numpy as np
    import ftk_amd
    from ftk_amd import _lib
    ctx, dom, recs = records_of(case)
    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=ftk_amd.CP_DTYPE)
    tags = np.ascontiguousarray(recs["tag"], dtype=np.uint64)
    st, sz = _lib.ll(dom[0]), _lib.ll(dom[1], fill=1)

    def trace(cur):
        _lib.check(L.ftkx_trace_curves_device(ctx._h, 2, st, sz, tags.ctypes.data, len(tags), 0, C.byref(cur)), ctx._h)

    def taken(out):
        ts = ftk_amd.TrajectorySet._from_c(out)
        L.ftkx_free_trajectories(C.byref(out))
        return ts

    def same(a, b):
        return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("offsets", "indices", "type", "loop", "id")) and np.array_equal(a.t.view(np.uint64), b.t.view(np.uint64))

    cur = _lib.Curves()
    trace(cur)

    def post(device):
        out = _lib.Trajectories()
        t0 = time.perf_counter()
        if device:
            rc = L.ftkx_post_process_curves_device(ctx._h, recs.ctypes.data, len(recs), C.byref(cur), C.byref(out))
        else:
            rc = L.ftkx_post_process_curves(recs.ctypes.data, len(recs), C.byref(cur), C.byref(out))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, ctx._h)
        return ms, (ctx.post_process_last_path() if device else 0), taken(out)

    def pass2(device):
        out, c2 = _lib.Trajectories(), _lib.Curves()
        t0 = time.perf_counter()
        if device:
            rc = L.ftkx_pass2_device(ctx._h, 2, st, sz, recs.ctypes.data, len(recs), None, C.byref(out))
        else:
            trace(c2)
            rc = L.ftkx_post_process_curves(recs.ctypes.data, len(recs), C.byref(c2), C.byref(out))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, ctx._h)
        path = (ctx.trace_last_path(), ctx.post_process_last_path() if device else 0)
        L.ftkx_free_curves(C.byref(c2))
        return ms, path, taken(out)

    if phases:
        for _ in range(3):
            post(True)
            sys.stderr.flush()
        pass2(True)
        return
    q = lambda v: tuple(float(np.percentile(v, p)) for p in (25, 50, 75))  # noqa: E731
    print("%s: %d records, %d points in %d curves; %d calls each after %d warm-up calls, interleaved" % (case, len(recs), cur.n_points, cur.n_curves, calls, warmup))
    ok = True
    for what, fn, names in (("post-processing", post, ("ftkx_post_process_curves", "ftkx_post_process_curves_device")),
                            ("pass 2", pass2, ("ftkx_trace_curves_device + ftkx_post_process_curves", "ftkx_pass2_device"))):
        for _ in range(warmup):
            fn(False); fn(True)
        a, b, identical = [], [], True
        for _ in range(calls):
            ms, pa, ra = fn(False); a.append(ms)
            ms, pb, rb = fn(True); b.append(ms)
            identical = identical and same(ra, rb)
        qa, qb = q(a), q(b)
        print("  %s: %d points in %d trajectories" % (what, len(ra.indices), len(ra)))
        print("    %-52s path %-6s median %.3f ms  (quartiles %.3f .. %.3f, min %.3f)" % (names[0], pa, qa[1], qa[0], qa[2], min(a)))
        print("    %-52s path %-6s median %.3f ms  (quartiles %.3f .. %.3f, min %.3f)" % (names[1], pb, qb[1], qb[0], qb[2], min(b)))
        print("    trajectories identical in every call: %s" % identical, flush=True)
        ok = ok and identical
    L.ftkx_free_curves(C.byref(cur))
    if not ok:
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each child may take")
    a = ap.parse_args()
    if a.case:
        one_case(a.case, a.phases, a.calls, a.warmup)
        return
    me = os.path.abspath(__file__)
    steps = []
    for case in ("C2", "C5"):
        steps.append("timeout -k 10 %d %s %s --case %s --calls %d --warmup %d" % (a.step_timeout, sys.executable, me, case, a.calls, a.warmup))
        steps.append("FTKX_POST_PROCESS_PHASES=1 FTKX_TRACE_PHASES=1 timeout -k 10 %d %s %s --case %s --phases" % (a.step_timeout, sys.executable, me, case))
    sys.exit(subprocess.call(" && ".join(steps), shell=True))


if __name__ == "__main__":
    main()
