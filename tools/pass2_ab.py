#!/usr/bin/env python3
"""Pass 2, A against B in one process: ftkx_trace_curves_tags_ctx (device phases, host walks) against ftkx_trace_curves_device (all of it
on the GPU), on the record sets of C2 (woven 1024^2 x 64) and C5 (double_gyre 2048 x 1024 x 128) as the library's own sweep delivers them.

    python tools/pass2_ab.py                 # every step as a child process under its own `timeout -k 10`, chained with &&
    python tools/pass2_ab.py --case C2       # one step: 5 warm-up calls of each, then 30 calls each, interleaved A B A B ...
    python tools/pass2_ab.py --case C2 --phases   # the device form's phases (FTKX_TRACE_PHASES: the host waits after each one)

Times are host clocks around the C call, which ends in a stream synchronise and returns the finished curves.  Printed: the median and the
quartiles of both, the path each took (ftkx_trace_last_path), and whether the curves are identical."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"C2": ("woven", (1024, 1024), 64, 1), "C5": ("double_gyre", (2048, 1024), 128, 2)}


def records_of(case):
    import numpy as np
    import torch
    import ftk_amd
    from ftk_amd import synthetic, tslab
    name, dims, nt, nv = CASES[case]
    scalar = nv == 1
    dev = torch.device("cuda", 0)
    ctx = ftk_amd.Context(2)
    dom = ([2 if scalar else 1] * 2, [d - (3 if scalar else 2) for d in dims])
    ctx.set_mesh(dom, dom, ([0, 0], list(dims)))
    ctx.set_options(jacobian_symmetric=int(scalar), derive_jacobian=1, tag_mode=ftk_amd.TAG_EXACT64)
    keep = []
    for t in range(nt):
        a = synthetic.generate(name, dims, t, nt, torch, dev)
        torch.cuda.synchronize()
        keep.append(a)
        (ctx.push_scalar_slice if scalar else ctx.push_slice)(t, a)
    rm = ctx.slices_prepare(range(nt), 0)
    factors = tslab.factors_from_resolutions([rm[t][0] for t in range(nt)])
    for t in range(nt):
        ctx.sweep_enqueue(t, ftk_amd.SCOPE_BOTH if t + 1 < nt else ftk_amd.SCOPE_ORDINAL, factors[t])
    recs = np.array(ctx.sweep_collect())
    for t in range(nt):
        ctx.drop_slice(t)
    del keep
    return ctx, dom, recs[np.argsort(recs["tag"], kind="stable")]


def one_case(case, phases, calls, warmup):
    import numpy as np
    from ftk_amd import _lib
    ctx, dom, recs = records_of(case)
    L = _lib.load()
    tags = np.ascontiguousarray(recs["tag"], dtype=np.uint64)
    st, sz = _lib.ll(dom[0]), _lib.ll(dom[1], fill=1)

    def call(device):
        out = _lib.Curves()
        t0 = time.perf_counter()
        if device:
            rc = L.ftkx_trace_curves_device(ctx._h, 2, st, sz, tags.ctypes.data, len(tags), 0, C.byref(out))
        else:
            rc = L.ftkx_trace_curves_tags_ctx(ctx._h, 2, st, sz, tags.ctypes.data, len(tags), C.byref(out))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, ctx._h)
        path = ctx.trace_last_path()
        res = (np.ctypeslib.as_array(out.offsets, shape=(out.n_curves + 1,)).copy(), np.ctypeslib.as_array(out.indices, shape=(max(1, out.n_points),))[:out.n_points].copy(),
               np.ctypeslib.as_array(out.loop, shape=(max(1, out.n_curves),))[:out.n_curves].copy(), int(out.n_special))
        L.ftkx_free_curves(C.byref(out))
        return ms, path, res

    if phases:
        for _ in range(3):
            call(True)
            sys.stderr.flush()
        return
    for _ in range(warmup):
        call(False); call(True)
    a, b = [], []
    for _ in range(calls):
        ms, pa, ra = call(False); a.append(ms)
        ms, pb, rb = call(True); b.append(ms)
    same = ra[3] == rb[3] and all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3]))
    q = lambda v: tuple(float(np.percentile(v, p)) for p in (25, 50, 75))  # noqa: E731
    qa, qb = q(a), q(b)
    print("%s: %d records, %d curves, %d special; %d calls each after %d warm-up calls, interleaved" % (case, len(tags), len(ra[2]), ra[3], calls, warmup))
    print("  ftkx_trace_curves_tags_ctx  path %d  median %.3f ms  (quartiles %.3f .. %.3f, min %.3f)" % (pa, qa[1], qa[0], qa[2], min(a)))
    print("  ftkx_trace_curves_device    path %d  median %.3f ms  (quartiles %.3f .. %.3f, min %.3f)" % (pb, qb[1], qb[0], qb[2], min(b)))
    print("  curves identical: %s" % same, flush=True)
    if not same:
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
        steps.append("FTKX_TRACE_PHASES=1 timeout -k 10 %d %s %s --case %s --phases" % (a.step_timeout, sys.executable, me, case))
    sys.exit(subprocess.call(" && ".join(steps), shell=True))


if __name__ == "__main__":
    main()
