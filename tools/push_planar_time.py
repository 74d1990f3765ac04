"""What the concat kernel (ftk_amd/csrc/concat_kernels.hip) costs next to a streaming kernel that moves the same bytes, and what a planar
push costs next to the host interleave it replaces.

    python tools/push_planar_time.py [--out FILE.json] [--quick] [--reps N] [--no-push]

Per case (T float32 / float64, NC 3 and 2; count = 512^3 vertices, --quick: 64^3), kernels alone, HIP events around every launch
(ftkx_debug_*_relaunch), `reps` >= 5 timed launches after 3 warm-up launches, concat and yardstick taken in turn (two rounds each):
  concat     ftkx_debug_concat_relaunch: NC planes of `count` elements in, NC * count doubles out
  yardstick  float32: ftkx_debug_widen_relaunch over NC * count floats; float64: ftkx_debug_adjust_relaunch, clamp only with lo = -inf and
             hi = +inf, out of place, over NC * count doubles -- the same bytes in and out, on the same device, in the same run
  rule       the store shape of the concat kernel is kept while its median is not above the yardstick's slowest repetition
The result of every concat launch is compared with torch's stack on the device.
Pushes (3D, 256^3 vertices; skipped with --no-push): median host time of ftkx_push_slice_planar of three fresh pageable planes against
np.stack(..., axis=-1) on the host followed by ftkx_push_slice, each ended by a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts), all_ms=[round(t, 4) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-push", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    reps, warm = max(5, a.reps), 3
    import numpy as np
    import torch
    import ftk_amd
    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to report without one"
    side = 64 if a.quick else 512
    count = side ** 3
    rows = []
    ctx = ftk_amd.Context(3)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    inf = float("inf")
    for tdtype, nc in ((torch.float32, 3), (torch.float32, 2), (torch.float64, 3), (torch.float64, 2)):
        f32 = tdtype == torch.float32
        size = 4 if f32 else 8
        planes = [torch.rand(count, dtype=tdtype, device="cuda") - 0.5 for _ in range(nc)]
        flat = torch.rand(nc * count, dtype=tdtype, device="cuda")            # the yardstick's source: the same bytes, one array
        dst = torch.empty(nc * count, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        k_ms, y_ms = [], []
        for _ in range(2):
            k_ms += ctx.debug_concat_relaunch([p.data_ptr() for p in planes], count, dst.data_ptr(), warm + reps, f32=f32)[warm:]
            assert torch.equal(dst.view(nc * count), torch.stack(planes, dim=-1).reshape(-1).double())
            if f32:
                y_ms += ctx.debug_widen_relaunch(flat.data_ptr(), nc * count, dst.data_ptr(), warm + reps)[warm:]
            else:
                y_ms += ctx.debug_adjust_relaunch(flat.data_ptr(), nc * count, dst.data_ptr(), warm + reps, clamp=(-inf, inf))[warm:]
        moved = nc * count * (size + 8)
        row = dict(T="float32" if f32 else "float64", nc=nc, count=count, bytes_moved=moved, concat=med(k_ms), yardstick=med(y_ms),
                   yardstick_kernel="widen" if f32 else "adjust, clamp only",
                   concat_median_over_yardstick_median=statistics.median(k_ms) / statistics.median(y_ms),
                   concat_median_over_yardstick_slowest=statistics.median(k_ms) / max(y_ms),
                   concat_bytes_per_second=moved / (statistics.median(k_ms) * 1e-3),
                   direct_form_kept=statistics.median(k_ms) <= max(y_ms), planar_counts=list(ctx.planar_counts()))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del planes, flat, dst
    ctx.close()
    if not a.no_push:
        side = 64 if a.quick else 256
        dims, n = (side, side, side), side ** 3
        base = [(np.random.default_rng(k).random(n, dtype=np.float32) - 0.5).reshape(dims) for k in range(3)]
        for dtype in (np.float32, np.float64):
            ctx = ftk_amd.Context(3)
            ctx.set_mesh(([1] * 3, [d - 2 for d in dims]), ([1] * 3, [d - 2 for d in dims]), ([0] * 3, list(dims)))

            def fresh():
                out = [np.empty(dims, dtype=dtype) for _ in range(3)]
                for o, b in zip(out, base):
                    o[...] = b
                return out

            def planar(i):
                p = fresh()
                t0 = time.perf_counter()
                ctx.push_slice_planar(i % 2, p)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            def host_interleave(i):
                p = fresh()
                t0 = time.perf_counter()
                ctx.push_slice(i % 2, np.stack(p, axis=-1))
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            ts = dict(planar=[], host_interleave_then_push=[])
            for i in range(2 + 7):
                for k, f in (("planar", planar), ("host_interleave_then_push", host_interleave)):
                    t = f(i)
                    if i >= 2:
                        ts[k].append(t)
            row = dict(push_dims=list(dims), T=np.dtype(dtype).name, planar=med(ts["planar"]), host_interleave_then_push=med(ts["host_interleave_then_push"]),
                       planar_counts=list(ctx.planar_counts()), upload_counts=list(ctx.upload_counts()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
