"""Device time of the temporal-smoothing kernel (ftk_amd/csrc/temporal_kernels.hip) next to a bare read of the same bytes.

    python tools/temporal_time.py [--out FILE.json] [--quick] [--reps N] [--only LABEL]

Per case: the kernel `reps` times by HIP events around every launch (ftkx_debug_temporal_relaunch) and `reps` times as
ftkx_temporal_combine by the host's clock (one launch and one wait per call); the first 3 of each dropped; median, minimum, maximum and
the quartiles of the rest.  The yardstick, in the same process on the same device: ftkx_debug_stream_read over as many bytes as the
kernel READS (8 bytes per element and DISTINCT array; the arrays lie back to back, so one call reads them all) -- one launch and one
wait as well, by the host's clock.  `kernel_over_read` compares the two host-clock medians: both carry the same launch and wake-up, which
the event times do not.  Bytes written (8 per element) are reported beside it: the read yardstick does not cover them.  `steady`: K
distinct arrays; `edge`: the first emission of a series, H = (K + 1) / 2 distinct arrays, the first one read by H taps; `finish`: the last
trailing emission, H distinct arrays, the last one read by H taps."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("512^3", 512 ** 3, 5), ("2048x1024", 2048 * 1024, 5)]
QUICK = [("128^3", 128 ** 3, 5), ("512x256", 512 * 256, 5)]


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), q1_ms=q[0], q3_ms=q[2], n=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=23)
    ap.add_argument("--only", help="one case by its label")
    a = ap.parse_args()
    import torch
    import ftk_amd
    rows = []
    for label, n, K in (QUICK if a.quick else CASES):
        if a.only and label != a.only:
            continue
        H = (K + 1) // 2
        ctx = ftk_amd.Context(3)
        src = torch.rand(K * n, dtype=torch.float64, device="cuda") - 0.5      # K arrays back to back
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        w = ftk_amd.gaussian_kernel1d(1.0, K)
        base = src.data_ptr()
        phases = {"steady": list(range(K)), "edge": [max(0, i - (H - 1)) for i in range(K)], "finish": [min(H - 1, i) for i in range(K)]}
        for phase, pattern in phases.items():
            distinct = len(set(pattern))
            ms = ctx.debug_temporal_relaunch([base + 8 * n * j for j in pattern], w, n, out.data_ptr(), a.reps)[3:]
            read_bytes, written = 8 * n * distinct, 8 * n
            ptrs = [base + 8 * n * j for j in pattern]
            hk = []                                   # the kernel as the yardstick is timed: one launch and one wait, by the host's clock
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.temporal_combine(ptrs, w, n, out.data_ptr())
                hk.append((time.perf_counter() - t0) * 1e3)
            hk = hk[3:]
            rd = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ftk_amd._lib.check(ctx._L.ftkx_debug_stream_read(ctx._h, C.c_void_p(base), read_bytes), ctx._h)
                rd.append((time.perf_counter() - t0) * 1e3)
            rd = rd[3:]
            k, r, h = spread(ms), spread(rd), spread(hk)
            rows.append(dict(case=label, elements=n, ksize=K, phase=phase, distinct_arrays=distinct, bytes_read=read_bytes, bytes_written=written, kernel=k, kernel_host_clock=h, bare_read=r,
                             kernel_over_read=h["median_ms"] / r["median_ms"], kernel_TBps=(read_bytes + written) / (k["median_ms"] * 1e-3) / 1e12,
                             read_TBps=read_bytes / (r["median_ms"] * 1e-3) / 1e12))
            print(json.dumps(rows[-1]), flush=True)
        ctx.close()
        del src, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
