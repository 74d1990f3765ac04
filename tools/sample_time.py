"""What sampling auxiliary scalar fields at critical points costs (ftk_amd/csrc/sample_kernels.hip), next to the sweep pass it follows.

    python tools/sample_time.py [--out FILE.json] [--quick] [--reps N]

Two record sets, each swept from resident device slices in this very process:
  c2   woven 1024^2 x 64 (bench.py's C2), the device-driven pass: about 6e4 records
  3d   moving_extremum_3d_overflow 72^3 x 4 under exact_only (the overflow regime: hits almost everywhere): more than 1e6 records
(--quick: 128^2 x 8 and 24^3 x 3, to rehearse the script.)  Two seeded fields of the slices' extent are lent as slots 1 and 2.  Reported per
set, each the median of N >= 21 runs after 3 warm-up runs, the variants taken in turn within one loop:
  kernel      ftkx_debug_sample_relaunch, one launch per run (HIP events): us per launch, ns per record
  call        ftkx_sample_aux on a copy of the records, host clock around the call (it ends in a wait for the stream): transfers included
  host_1 / host_16   the host build of sample_steps.hpp (tests/hostcheck/sample_host.cpp) on the same records and host copies of the same
              arrays, one thread and sixteen
  sweep       ftkx_sweep_series over the same steps with the masks dropped first (the whole pass is redone), host clock around the call.
              No sweep kernel, launch or host path differs from the commit before this feature: its time here is that commit's.
The kernel's result is held to the host build's, bit for bit, before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(ts, scale=1.0):
    return dict(median=statistics.median(ts) * scale, min=min(ts) * scale, max=max(ts) * scale, n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    reps, warm = max(21, a.reps), 3
    import numpy as np
    import torch
    import ftk_amd
    import sample_cases as SC
    from ftk_amd import synthetic
    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to report without one"
    sets = [("c2", 2, "woven", (128, 128) if a.quick else (1024, 1024), 8 if a.quick else 64, False),
            ("3d", 3, "moving_extremum_3d_overflow", (24, 24, 24) if a.quick else (72, 72, 72), 3 if a.quick else 4, True)]
    rows = []
    for label, nd, case, dims, nt, exact_only in sets:
        dom = ([2] * nd, [d - 3 for d in dims])
        ctx = ftk_amd.Context(nd)
        ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
        ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=ftk_amd.TAG_EXACT64, exact_only=int(exact_only))
        S = [synthetic.generate(case, dims, k, nt, torch, "cuda") for k in range(nt)]
        gen = torch.Generator(device="cuda"); gen.manual_seed(7)
        A = [[(torch.rand(S[0].shape, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 2e3 for _ in range(nt)] for _ in range(2)]
        torch.cuda.synchronize()
        for k in range(nt):
            ctx.push_scalar_slice(k, S[k])
            ctx.push_aux_slice(k, 1, A[0][k]); ctx.push_aux_slice(k, 2, A[1][k])
        ts = np.arange(nt, dtype=np.int32)
        scopes = np.array([ftk_amd.SCOPE_BOTH] * (nt - 1) + [ftk_amd.SCOPE_ORDINAL], dtype=np.int32)
        recs = ctx.sweep_series(ts, scopes)[0]
        n = len(recs)
        row = dict(set=label, case=case, dims=list(dims), timesteps=nt, exact_only=exact_only, records=n, series_path=ctx.series_last_path()[0])
        # the kernel against the host build, before anything is timed
        g = dict(nd=nd, nv=1, dims=list(dims), steps=[s.cpu().numpy() for s in S])
        hostA = [[x.cpu().numpy() for x in A[s]] for s in range(2)]
        got = ctx.sample_aux(recs.copy())
        h1, h2, ok, bad = SC.host_sample(g, SC.TAG_EXACT64, recs["tag"], recs["aux"], A1=hostA[0], A2=hostA[1], nthreads=16)
        assert bad == 0 and SC.same_doubles(got["scalar"][:, 1], h1) and SC.same_doubles(got["scalar"][:, 2], h2), "the kernel's result is not the host build's"
        scratch = recs.copy()

        def kernel():
            return ctx.debug_sample_relaunch(recs, 1)[0]

        def call():
            t0 = time.perf_counter(); ctx.sample_aux(scratch); return (time.perf_counter() - t0) * 1e3

        def host(nthreads):
            t0 = time.perf_counter()
            SC.host_sample(g, SC.TAG_EXACT64, recs["tag"], recs["aux"], A1=hostA[0], A2=hostA[1], nthreads=nthreads)
            return (time.perf_counter() - t0) * 1e3

        def sweep():
            ctx.invalidate_masks()
            torch.cuda.synchronize()
            t0 = time.perf_counter(); ctx.sweep_series(ts, scopes, copy=False); return (time.perf_counter() - t0) * 1e3

        variants = {"kernel": kernel, "call": call, "host_1": lambda: host(1), "host_16": lambda: host(16), "sweep": sweep}
        times = {k: [] for k in variants}
        for i in range(warm + reps):
            for k, f in variants.items():
                t = f()
                if i >= warm:
                    times[k].append(t)
        m = {k: statistics.median(v) for k, v in times.items()}
        row["kernel_us_per_launch"] = med(times["kernel"], 1e3)
        row["kernel_ns_per_record"] = m["kernel"] * 1e6 / max(1, n)
        for k in ("call", "host_1", "host_16", "sweep"):
            row[k + "_ms"] = med(times[k])
        row["call_ns_per_record"] = m["call"] * 1e6 / max(1, n)
        row["call_over_sweep"] = m["call"] / m["sweep"]
        row["call_minus_kernel_ms"] = m["call"] - m["kernel"]
        row["bytes_up"] = 16 * n
        row["bytes_down"] = 16 * n
        ctx.close()
        del S, A
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
