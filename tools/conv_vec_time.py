"""Device time of the vector smoothing's kernel (ftk_amd/csrc/conv_vec_kernels.hip) next to the route a user had without it.

    python tools/conv_vec_time.py [--out FILE.json] [--quick]

Per case -- random input, nd components -- the median (and min - max) of 20 launches after 3 warm-up launches, by HIP events around every
launch: the new kernel from the interleaved array and from planes (ftkx_debug_conv_vec_relaunch), and in the same process the old route,
whose kernels this build has unchanged:
    (a) the nd launches of ftkx_conv2D / ftkx_conv3D on de-interleaved planes alone (ftkx_debug_conv_relaunch; launch i of every plane added up),
    (b) the same plus ftkx_concat of the smoothed planes (ftkx_debug_concat_relaunch),
    (c) the same plus the de-interleave, done the way a torch user does it: one strided copy per component (events on torch's stream).
ok: the new kernel's median (interleaved) is not above (c)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [((4096, 4096), 3), ((4096, 4096), 5), ((256, 256, 256), 3), ((256, 256, 256), 5), ((512, 512, 512), 3), ((512, 512, 512), 5)]
QUICK = [((1024, 1024), 3), ((128, 128, 128), 3), ((128, 128, 128), 5)]
WARM, REPS = 3, 20


def spread(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


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
        V = torch.rand(n * nd, dtype=torch.float64, device="cuda") - 0.5
        out = torch.empty(n * nd, dtype=torch.float64, device="cuda")
        planes = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(nd)]
        smoothed = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(nd)]
        w = ftk_amd.gaussian_kernel(nd, 1.0, k)

        # (c)'s own part: the de-interleave, timed on torch's stream
        split = []
        for i in range(WARM + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(nd):
                planes[c].copy_(V.view(n, nd)[:, c])
            e1.record()
            torch.cuda.synchronize()
            split.append(e0.elapsed_time(e1))
        split = split[WARM:]
        per_plane = [ctx.debug_conv_relaunch(planes[c].data_ptr(), dims, w, k, smoothed[c].data_ptr(), WARM + REPS)[WARM:] for c in range(nd)]
        ra = [sum(p[i] for p in per_plane) for i in range(REPS)]
        concat = ctx.debug_concat_relaunch([s.data_ptr() for s in smoothed], n, out.data_ptr(), WARM + REPS)[WARM:]
        rb = [ra[i] + concat[i] for i in range(REPS)]
        rc = [rb[i] + split[i] for i in range(REPS)]
        old = out.clone()
        out.fill_(777.0)
        torch.cuda.synchronize()
        inter = ctx.debug_conv_vec_relaunch([V.data_ptr()], dims, w, k, out.data_ptr(), WARM + REPS)[WARM:]
        same = bool(torch.equal(out.view(torch.int64), old.view(torch.int64)))
        planar = ctx.debug_conv_vec_relaunch([p.data_ptr() for p in planes], dims, w, k, out.data_ptr(), WARM + REPS, planar=True)[WARM:]
        same = same and bool(torch.equal(out.view(torch.int64), old.view(torch.int64)))
        row = dict(dims=list(dims), ksize=k, conv_vec_interleaved=spread(inter), conv_vec_planar=spread(planar), route_a_scalar_launches=spread(ra),
                   route_b_plus_concat=spread(rb), route_c_plus_deinterleave=spread(rc), same_bytes_as_the_old_route=same,
                   ok=statistics.median(inter) <= statistics.median(rc), within_spread_of_a=min(ra) <= statistics.median(inter) <= max(ra) or statistics.median(inter) < min(ra))
        rows.append(row)
        print(json.dumps(row), flush=True)
        ctx.close()
        del V, out, planes, smoothed, old
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(cases=rows), f, indent=1)


if __name__ == "__main__":
    main()
