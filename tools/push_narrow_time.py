"""What a uint8 / int16 / float16 snapshot costs on its way into a context, next to the float32 and FP64 pushes of the same values
(ftk_amd/csrc/narrow_kernels.hip, widen_kernels.hip, upload.cpp).

    python tools/push_narrow_time.py [--out FILE.json] [--quick] [--reps N]

Per size (256^3 and 512^3; --quick: 64^3), the median of N >= 20 timed pushes after 3 warm-up pushes, the variants taken in turn within one
loop so that whatever else the box does meets all of them alike.  A push is timed by the host clock from the call to the end of a device
synchronise behind it.  The values are integers of 0 .. 255, exact in every one of the types.
  a  ftkx_push_scalar_slice of a FRESH pageable float64 array (allocated and filled for this push, like a reader does): the yardstick
  b  ftkx_push_scalar_slice_f32 of the same values as a fresh pageable float32 array
  n  ftkx_push_scalar_slice_typed (keep_dtype=True) of the same values as fresh pageable uint8, int16 and float16 arrays
  c  what a user of these types had to do before: astype(float64) on the host, then a
  d  the narrow kernel alone per element size (ftkx_debug_narrow_relaunch, HIP events), the widen kernel alone on the same count -- twice,
     the spread between its two medians being what "not slower" is read against -- and a bare read of the narrow kernel's source bytes
     (ftkx_debug_stream_read, events on the same stream)
Bytes over the link per push: a 8 per value, b 4, int16 and float16 2, uint8 1."""
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
    narrow = (("uint8", np.uint8, ftk_amd.DTYPE_U8), ("int16", np.int16, ftk_amd.DTYPE_I16), ("float16", np.float16, ftk_amd.DTYPE_F16))
    rows = []
    for side in ((64,) if a.quick else (256, 512)):
        dims = (side, side, side)
        n = side ** 3
        base = np.random.default_rng(side).integers(0, 256, size=n, dtype=np.uint8).reshape(dims)
        row = dict(dims=list(dims), bytes_per_push=dict(float64=8 * n, float32=4 * n, int16=2 * n, float16=2 * n, uint8=n))

        def fresh(dtype):
            x = np.empty(dims, dtype=dtype)
            x[...] = base
            return x

        def timed(ctx, i, make, prepare=None, keep_dtype=False):
            x = make()
            t0 = time.perf_counter()
            if prepare:
                x = prepare(x)
            ctx.push_scalar_slice(i % 2, x, keep_dtype=keep_dtype)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        ctx = ftk_amd.Context(3)
        ctx.set_mesh(([2] * 3, [d - 3 for d in dims]), ([2] * 3, [d - 3 for d in dims]), ([0] * 3, list(dims)))
        variants = {"a_f64_pageable": lambda i: timed(ctx, i, lambda: fresh(np.float64)),
                    "b_f32_pageable": lambda i: timed(ctx, i, lambda: fresh(np.float32))}
        for name, dtype, _ in narrow:
            variants["n_%s_pageable" % name] = lambda i, dtype=dtype: timed(ctx, i, lambda: fresh(dtype), keep_dtype=True)
            variants["c_%s_astype_then_f64" % name] = lambda i, dtype=dtype: timed(ctx, i, lambda: fresh(dtype), lambda x: x.astype(np.float64))
        ts = {k: [] for k in variants}
        for i in range(warm + reps):
            for k, f in variants.items():
                t = f(i)
                if i >= warm:
                    ts[k].append(t)
        row["push"] = {k: med(v) for k, v in ts.items()}
        row["narrow_counts"] = list(ctx.narrow_counts())
        row["f32_counts"] = list(ctx.f32_counts())
        row["upload_counts"] = list(ctx.upload_counts())
        ctx.close()
        # d: the kernels alone, and a bare read of the narrow kernel's source
        ctx = ftk_amd.Context(3)
        st = torch.cuda.current_stream()
        ctx.set_stream(st.cuda_stream)
        dst = torch.empty(n, dtype=torch.float64, device="cuda")
        src32 = torch.from_numpy(base.reshape(-1).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        kernels = {}
        w1 = ctx.debug_widen_relaunch(src32.data_ptr(), n, dst.data_ptr(), warm + reps)[warm:]
        for name, dtype, code in narrow:
            src = torch.from_numpy(base.reshape(-1).astype(dtype)).cuda()
            torch.cuda.synchronize()
            k_ms = ctx.debug_narrow_relaunch(src.data_ptr(), code, n, dst.data_ptr(), warm + reps)[warm:]
            assert torch.equal(dst, src.double())
            r_ms = []
            for i in range(warm + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                ftk_amd._lib.check(ctx._L.ftkx_debug_stream_read(ctx._h, src.data_ptr(), src.element_size() * n), ctx._h)
                e1.record(st)
                torch.cuda.synchronize()
                if i >= warm:
                    r_ms.append(e0.elapsed_time(e1))
            kernels[name] = dict(narrow_kernel=med(k_ms), bare_read_of_source=med(r_ms), bytes_per_second=(src.element_size() + 8) * n / (statistics.median(k_ms) * 1e-3))
            del src
        w2 = ctx.debug_widen_relaunch(src32.data_ptr(), n, dst.data_ptr(), warm + reps)[warm:]
        assert torch.equal(dst, src32.double())
        row["d_widen_kernel_first"] = med(w1)
        row["d_widen_kernel_again"] = med(w2)
        row["d_widen_spread_ms"] = abs(statistics.median(w1) - statistics.median(w2))
        row["d_kernels"] = kernels
        for name in kernels:
            kernels[name]["over_widen_kernel"] = kernels[name]["narrow_kernel"]["median_ms"] / min(statistics.median(w1), statistics.median(w2))
        ctx.close()
        del src32, dst
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
