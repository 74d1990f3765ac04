"""What a float32 snapshot costs on its way into a context, next to the FP64 push it replaces (ftk_amd/csrc/widen_kernels.hip, upload.cpp).

    python tools/push_f32_time.py [--out FILE.json] [--quick] [--reps N]

Per size (256^3 and 512^3; --quick: 64^3), the median of N >= 20 timed pushes after 3 warm-up pushes, the variants taken in turn within one
loop so that whatever else the box does meets all of them alike.  A push is timed by the host clock from the call to the end of a device
synchronise behind it: the call returns when the caller's array has been read, the widen kernel or the convolution may still run then.
  a  ftkx_push_scalar_slice of a FRESH pageable float64 array (allocated and filled for this push, like a reader does): the yardstick
  b  ftkx_push_scalar_slice_f32 of the same values as float32 -- a fresh pageable array, and a pinned one
  c  what a float32 user had to do before: astype(float64) on the host, then a
  d  the widen kernel alone (ftkx_debug_widen_relaunch, HIP events) over a bare read of the same 12 bytes per element
     (ftkx_debug_stream_read, events on the same stream)
  e  a and b (pageable) with ksize 5 spatial smoothing set
Bytes over the link per push: a 8 per value, b 4."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    reps, warm = max(20, a.reps), 3
    import numpy as np
    import torch
    import ftk_amd
    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to report without one"
    rows = []
    for side in ((64,) if a.quick else (256, 512)):
        dims = (side, side, side)
        n = side ** 3
        base32 = (np.random.default_rng(side).random(n, dtype=np.float32) - 0.5).reshape(dims)
        pinned32 = torch.from_numpy(base32).pin_memory()
        row = dict(dims=list(dims), bytes_per_push=dict(float64=8 * n, float32=4 * n))

        def fresh(dtype):
            x = np.empty(dims, dtype=dtype)
            x[...] = base32
            return x

        def timed(ctx, i, make, prepare=None):
            x = make()
            t0 = time.perf_counter()
            if prepare:
                x = prepare(x)
            ctx.push_scalar_slice(i % 2, x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for label, smoothing in (("plain", None), ("ksize5", (1.0, 5))):
            ctx = ftk_amd.Context(3)
            ctx.set_mesh(([2] * 3, [d - 3 for d in dims]), ([2] * 3, [d - 3 for d in dims]), ([0] * 3, list(dims)))
            if smoothing:
                ctx.set_spatial_smoothing(*smoothing)
            variants = {"a_f64_pageable": lambda i: timed(ctx, i, lambda: fresh(np.float64)),
                        "b_f32_pageable": lambda i: timed(ctx, i, lambda: fresh(np.float32))}
            if not smoothing:
                variants["b_f32_pinned"] = lambda i: timed(ctx, i, lambda: pinned32)
                variants["c_astype_then_f64"] = lambda i: timed(ctx, i, lambda: fresh(np.float32), lambda x: x.astype(np.float64))
            ts = {k: [] for k in variants}
            for i in range(warm + reps):
                for k, f in variants.items():
                    t = f(i)
                    if i >= warm:
                        ts[k].append(t)
            row[label] = {k: med(v) for k, v in ts.items()}
            row[label]["f32_counts"] = list(ctx.f32_counts())
            row[label]["upload_counts"] = list(ctx.upload_counts())
            ctx.close()
        # d: the kernel alone against a bare read of 12 bytes per element
        ctx = ftk_amd.Context(3)
        st = torch.cuda.current_stream()
        ctx.set_stream(st.cuda_stream)
        src = torch.from_numpy(base32.reshape(-1)).cuda()
        dst = torch.empty(n, dtype=torch.float64, device="cuda")
        both = torch.empty(3 * n, dtype=torch.float32, device="cuda")          # 12 bytes per element
        torch.cuda.synchronize()
        k_ms = ctx.debug_widen_relaunch(src.data_ptr(), n, dst.data_ptr(), warm + reps)[warm:]
        r_ms = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ftk_amd._lib.check(ctx._L.ftkx_debug_stream_read(ctx._h, both.data_ptr(), 12 * n), ctx._h)
            e1.record(st)
            torch.cuda.synchronize()
            if i >= warm:
                r_ms.append(e0.elapsed_time(e1))
        assert torch.equal(dst, src.double())
        row["d_widen_kernel"] = med(k_ms)
        row["d_bare_read_12B"] = med(r_ms)
        row["d_bare_read_over_kernel"] = statistics.median(r_ms) / statistics.median(k_ms)
        row["d_kernel_bytes_per_second"] = 12 * n / (statistics.median(k_ms) * 1e-3)
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
