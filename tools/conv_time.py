"""Device time of the spatial-smoothing kernel (ftk_amd/csrc/conv_kernels.hip) and what a smoothed push costs over a plain one.

    python tools/conv_time.py [--out FILE.json] [--quick]

Per case: the median of 20 launches after 3 warm-up launches, by HIP events around every launch (ftkx_debug_conv_relaunch), next to the
FP64-issue floor of the kernel's own arithmetic: per output ksize^nd multiplies and ksize^nd adds (the reference's order forbids fusing
them), a wavefront's FP64 instruction taking 4 cycles on one of 4 SIMDs of 256 CUs at 2.4 GHz -- 78.6 TFLOP/s with an FMA counted as two,
the data sheet's figure, not measured here.  Then ftkx_push_scalar_slice of a device array (on_device = 2) with and without smoothing."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LANE_OPS_PER_SECOND = 256 * 4 * 16 * 2.4e9      # FP64 VALU lane-instructions per second of the whole part

CASES = [((256, 256, 256), 3), ((256, 256, 256), 5), ((512, 512, 512), 3), ((512, 512, 512), 5), ((1024, 1024), 5), ((4096, 4096), 5)]
QUICK = [((128, 128, 128), 3), ((128, 128, 128), 5), ((1024, 1024), 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    import ftk_amd
    rows = []
    for dims, k in (QUICK if a.quick else CASES):
        nd = len(dims)
        ctx = ftk_amd.Context(nd)
        n = 1
        for d in dims:
            n *= d
        src = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        w = ftk_amd.gaussian_kernel(nd, 1.0, k)
        ms = ctx.debug_conv_relaunch(src.data_ptr(), dims, w, k, out.data_ptr(), 23)[3:]
        floor = n * 2 * k ** nd / LANE_OPS_PER_SECOND * 1e3
        rows.append(dict(dims=list(dims), ksize=k, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), issue_floor_ms=floor,
                         times_floor=statistics.median(ms) / floor, outputs_per_second=n / (statistics.median(ms) * 1e-3)))
        print(json.dumps(rows[-1]), flush=True)
        ctx.close()
        del src, out
    # a smoothed push over a plain one: a device array, copied (2) or convolved into the context's buffer
    dims = (128, 128, 128) if a.quick else (512, 512, 512)
    n = dims[0] * dims[1] * dims[2]
    src = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
    torch.cuda.synchronize()
    push = {}
    for label, smoothing in (("plain", None), ("ksize3", (1.0, 3)), ("ksize5", (1.0, 5))):
        ctx = ftk_amd.Context(3)
        ctx.set_mesh(([2] * 3, [d - 3 for d in dims]), ([2] * 3, [d - 3 for d in dims]), ([0] * 3, list(dims)))
        if smoothing:
            ctx.set_spatial_smoothing(*smoothing)
        ts = []
        for i in range(9):
            t0 = time.perf_counter()
            ctx.push_scalar_slice(i % 2, src, on_device=2)
            ts.append((time.perf_counter() - t0) * 1e3)
        push[label] = dict(median_ms=statistics.median(ts[2:]), min_ms=min(ts[2:]), first_ms=ts[0])
        ctx.close()
    print(json.dumps(dict(push_dims=list(dims), push=push)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(kernel=rows, push_dims=list(dims), push=push), f, indent=1)


if __name__ == "__main__":
    main()
