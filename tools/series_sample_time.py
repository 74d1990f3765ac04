"""What it costs, and saves, to have the series pass sample its own records (ftkx_set_series_sampling; series_sample_kernel in
ftk_amd/csrc/sample_kernels.hip) instead of calling ftkx_sample_aux on the finished records.

    python tools/series_sample_time.py [--out FILE.json] [--quick] [--reps N] [--only a,b,c]

One process on one GPU; per part the variants are taken in turn within one loop, 3 warm-up runs, then the median [min - max] of N >= 21 runs.
Results are held equal byte for byte before anything is timed.
  (a) C2, woven 1024^2 x 64, two lent FP64 fields, both slots, masks dropped before every run:
        armed        the armed ftkx_sweep_series (records come back filled)
        pass_call    the unarmed ftkx_sweep_series followed by ftkx_sample_aux -- the way before the switch, same binary
        pass         the unarmed ftkx_sweep_series alone: armed - pass is what arming costs (records left on the device, the copy kernel, the
                     kernel chain in place of the fused tail where that applies, the sample kernel)
  (b) 3D moving_extremum_3d_overflow 72^3 x 4 under exact_only -- the host-driven batch, so the armed pass samples behind the batch inside
      the call (ftkx_series_sampled: where = 2): armed against pass_call; the expectation is equal
  (c) the streaming tracker at 512^3 (moving_extremum_3d) with one component, set_sampling_in_pass(True): collected per step, deferred
      depth 1 and depth 4 -- ms per step over the whole run, one run per repetition
(--quick: 128^2 x 8, 24^3 x 3 and 48^3, to rehearse the script.)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(ts, scale=1.0):
    return dict(median=statistics.median(ts) * scale, min=min(ts) * scale, max=max(ts) * scale, n=len(ts))


def alternate(variants, warm, reps):
    times = {k: [] for k in variants}
    for i in range(warm + reps):
        for k, f in variants.items():
            t = f()
            if i >= warm:
                times[k].append(t)
    return times


def series_part(label, nd, case, dims, nt, exact_only, warm, reps):
    import numpy as np
    import torch
    import ftk_amd
    from ftk_amd import synthetic
    dom = ([2] * nd, [d - 3 for d in dims])
    S = [synthetic.generate(case, dims, k, nt, torch, "cuda") for k in range(nt)]
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    A = [[(torch.rand(S[0].shape, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 2e3 for _ in range(nt)] for _ in range(2)]
    torch.cuda.synchronize()
    ctxs = {}
    for which in ("armed", "plain"):
        ctx = ftk_amd.Context(nd)
        ctx.set_mesh(dom, dom, ([0] * nd, list(dims)))
        ctx.set_options(jacobian_symmetric=1, derive_jacobian=1, tag_mode=ftk_amd.TAG_EXACT64, exact_only=int(exact_only))
        ctx.set_series_sampling(which == "armed")
        for k in range(nt):
            ctx.push_scalar_slice(k, S[k])
            ctx.push_aux_slice(k, 1, A[0][k], on_device=1); ctx.push_aux_slice(k, 2, A[1][k], on_device=1)
        ctxs[which] = ctx
    ts = np.arange(nt, dtype=np.int32)
    scopes = np.array([ftk_amd.SCOPE_BOTH] * (nt - 1) + [ftk_amd.SCOPE_ORDINAL], dtype=np.int32)
    # twice each: the second pass has the buffers and the hit count of the first
    for _ in range(2):
        ctxs["armed"].invalidate_masks(); got = ctxs["armed"].sweep_series(ts, scopes)[0]
        ctxs["plain"].invalidate_masks(); want = ctxs["plain"].sample_aux(ctxs["plain"].sweep_series(ts, scopes)[0])
    assert got.tobytes() == want.tobytes(), "the armed pass is not the pass followed by the call"
    row = dict(part=label, case=case, dims=list(dims), timesteps=nt, exact_only=exact_only, records=len(got), armed_path=ctxs["armed"].series_last_path()[0],
               plain_path=ctxs["plain"].series_last_path()[0], sampled=list(ctxs["armed"].series_sampled()), workgroups=ctxs["armed"].series_sample_counts()[2])

    def run(which, call):
        ctx = ctxs[which]
        ctx.invalidate_masks()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ctx.sweep_series(ts, scopes, copy=False)[0]
        if call:
            ctx.sample_aux(r if r.flags.writeable else r.copy())      # (in the context's own record buffer where the view allows it)
        return (time.perf_counter() - t0) * 1e3

    times = alternate({"armed": lambda: run("armed", False), "pass_call": lambda: run("plain", True), "pass": lambda: run("plain", False)}, warm, reps)
    for k, v in times.items():
        row[k + "_ms"] = med(v)
    m = {k: statistics.median(v) for k, v in times.items()}
    row["armed_minus_pass_ms"] = m["armed"] - m["pass"]
    row["pass_call_minus_armed_ms"] = m["pass_call"] - m["armed"]
    row["spread_ms"] = max(max(times["armed"]) - min(times["armed"]), max(times["pass_call"]) - min(times["pass_call"]))
    row["armed_faster_beyond_spread"] = bool(row["pass_call_minus_armed_ms"] > row["spread_ms"])
    for ctx in ctxs.values():
        ctx.close()
    return row


def tracker_part(dims, nsteps, warm, reps):
    import torch
    import ftk_amd
    from ftk_amd import synthetic
    S = [synthetic.generate("moving_extremum_3d", dims, k, nsteps, torch, "cuda") for k in range(nsteps)]
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    A = [(torch.rand(S[0].shape, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 2e3 for _ in range(nsteps)]
    torch.cuda.synchronize()

    def run(depth, in_pass=True):
        tr = ftk_amd.CriticalPointTracker3DRegular()
        tr.set_scalar_field_source(ftk_amd.SOURCE_GIVEN); tr.set_vector_field_source(ftk_amd.SOURCE_DERIVED)
        tr.set_jacobian_field_source(ftk_amd.SOURCE_DERIVED); tr.set_jacobian_symmetric(True)
        tr.set_domain([2, 2, 2], [d - 3 for d in dims]); tr.set_array_domain([0, 0, 0], list(dims))
        tr.set_tag_mode(ftk_amd.TAG_EXACT64)      # (at 512^3 the reference's int32 tags wrap: neither sampler decodes them)
        tr.set_scalar_components(["s", "a"])
        tr.set_sampling_in_pass(in_pass)
        tr.initialize()
        if depth:
            tr.set_deferred_collection(True, depth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(nsteps):
            tr.push_scalar_field_snapshot(S[k], components=[A[k]])
            if k:
                tr.advance_timestep()
        tr.update_timestep()
        recs = tr.get_critical_points()[0]
        ms = (time.perf_counter() - t0) * 1e3 / nsteps
        tr.close()
        return ms, recs

    base = run(0, in_pass=False)[1]
    for depth in (0, 1, 4):
        assert run(depth)[1].tobytes() == base.tobytes(), "the tracker's points differ at depth %d" % depth
    times = alternate({"per_step": lambda: run(0)[0], "deferred_1": lambda: run(1)[0], "deferred_4": lambda: run(4)[0], "records_pass": lambda: run(0, in_pass=False)[0]}, warm, reps)
    row = dict(part="c", case="moving_extremum_3d", dims=list(dims), steps=nsteps, points=len(base))
    for k, v in times.items():
        row[k + "_ms_per_step"] = med(v)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    reps, warm = max(21, a.reps), 3
    import torch
    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to report without one"
    rows = []
    only = a.only.split(",")
    if "a" in only:
        rows.append(series_part("a", 2, "woven", (128, 128) if a.quick else (1024, 1024), 8 if a.quick else 64, False, warm, reps))
        print(json.dumps(rows[-1]), flush=True)
    if "b" in only:
        rows.append(series_part("b", 3, "moving_extremum_3d_overflow", (24, 24, 24) if a.quick else (72, 72, 72), 3 if a.quick else 4, True, warm, reps))
        print(json.dumps(rows[-1]), flush=True)
    if "c" in only:
        rows.append(tracker_part((48, 48, 48) if a.quick else (512, 512, 512), 8 if a.quick else 16, warm, reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
