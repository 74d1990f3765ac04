"""What perturbation and clamp cost on the device, next to what they cost on the host before (ftk_amd/csrc/adjust_kernels.hip).

    python tools/adjust_time.py [--out FILE.json] [--quick] [--reps N]

Per size (256^3 and 512^3; --quick: 64^3), the median of N >= 21 timed pushes after 3 warm-up pushes, the variants taken in turn within one
loop so that whatever else the box does meets all of them alike.  A push is timed by the host clock from the call to the end of a device
synchronise behind it; the snapshot itself (a pageable float64 array) exists before the clock starts.
  a  the way without this feature: x + rng.normal(0, sigma, n), np.clip on the host (numpy, one thread), then ftkx_push_scalar_slice: the
     yardstick
  b  ftkx_push_scalar_slice with ftkx_set_perturbation and ftkx_set_clamp on
  c  ftkx_push_scalar_slice with both off
  d  the kernel alone (ftkx_debug_adjust_relaunch, HIP events), FP64 out of place: clamp only, perturb only, both -- over a bare read of the
     same 16 bytes per element (ftkx_debug_stream_read, events on the same stream)
The condition is b <= a; b - c (what the adjust kernel adds to a push) and d are reported."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIGMA, SEED, CLAMP = 0.05, 12345, (-0.4, 0.4)


def med(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


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
    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to report without one"
    rows = []
    for side in ((64,) if a.quick else (256, 512)):
        dims = (side, side, side)
        n = side ** 3
        base = (np.random.default_rng(side).random(n) - 0.5).reshape(dims)
        rng = np.random.default_rng(SEED)
        row = dict(dims=list(dims), sigma=SIGMA, clamp=list(CLAMP))

        def context(adjust):
            ctx = ftk_amd.Context(3)
            ctx.set_mesh(([2] * 3, [d - 3 for d in dims]), ([2] * 3, [d - 3 for d in dims]), ([0] * 3, list(dims)))
            if adjust:
                ctx.set_perturbation(SIGMA, SEED)
                ctx.set_clamp(*CLAMP)
            return ctx

        plain, adjusting = context(False), context(True)

        def timed(ctx, i, prepare=None):
            t0 = time.perf_counter()
            x = prepare(base) if prepare else base
            ctx.push_scalar_slice(i % 2, x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def on_host(x):
            return np.clip(x + rng.normal(0.0, SIGMA, x.shape), CLAMP[0], CLAMP[1])

        variants = {"a_host_adjust_then_push": lambda i: timed(plain, i, on_host),
                    "b_push_adjusting": lambda i: timed(adjusting, i),
                    "c_push_plain": lambda i: timed(plain, i)}
        ts = {k: [] for k in variants}
        for i in range(warm + reps):
            for k, f in variants.items():
                t = f(i)
                if i >= warm:
                    ts[k].append(t)
        row["push"] = {k: med(v) for k, v in ts.items()}
        m = {k: statistics.median(v) for k, v in ts.items()}
        row["b_over_a"] = m["b_push_adjusting"] / m["a_host_adjust_then_push"]
        row["b_minus_c_ms"] = m["b_push_adjusting"] - m["c_push_plain"]
        row["b_not_slower_than_a"] = bool(m["b_push_adjusting"] <= m["a_host_adjust_then_push"])
        row["adjust_counts"] = list(adjusting.adjust_counts())
        plain.close(); adjusting.close()
        # d: the kernel alone against a bare read of 16 bytes per element
        ctx = ftk_amd.Context(3)
        st = torch.cuda.current_stream()
        ctx.set_stream(st.cuda_stream)
        src = torch.from_numpy(base.reshape(-1)).cuda()
        dst = torch.empty(n, dtype=torch.float64, device="cuda")
        both = torch.empty(2 * n, dtype=torch.float64, device="cuda")          # 16 bytes per element
        torch.cuda.synchronize()
        kernels = {"d_clamp_only": dict(clamp=CLAMP), "d_perturb_only": dict(sigma=SIGMA, seed=SEED), "d_both": dict(sigma=SIGMA, seed=SEED, clamp=CLAMP)}
        k_ms = {k: [] for k in kernels}
        r_ms = []
        for i in range(warm + reps):
            for k, kw in kernels.items():
                t = ctx.debug_adjust_relaunch(src.data_ptr(), n, dst.data_ptr(), 1, t=i, **kw)[0]
                if i >= warm:
                    k_ms[k].append(t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ftk_amd._lib.check(ctx._L.ftkx_debug_stream_read(ctx._h, both.data_ptr(), 16 * n), ctx._h)
            e1.record(st)
            torch.cuda.synchronize()
            if i >= warm:
                r_ms.append(e0.elapsed_time(e1))
        row["d_bare_read_16B"] = med(r_ms)
        for k, v in k_ms.items():
            row[k] = med(v)
            row[k]["bytes_per_second"] = 16 * n / (statistics.median(v) * 1e-3)
            row[k]["elements_per_second"] = n / (statistics.median(v) * 1e-3)
            row[k]["over_bare_read"] = statistics.median(v) / statistics.median(r_ms)
        ctx.close()
        del src, dst, both
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
