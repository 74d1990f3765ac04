"""Regenerates tests/golden/temporal/*.npz from the REAL reference: tests/golden/temporal/temporal_driver.cpp (this repository's text) is
compiled in a scratch directory against the reference's headers and a config.hh made by oracle/gen_config.cmake, and run once per case.

    python tests/golden/temporal/make_golden_temporal.py [REFERENCE_ROOT]

Every file holds: dims (fastest first; a vector case's first entry is its number of components), sigma, ksize, input (N raw arrays),
weights (the reference's gaussian_kernel), output (every array ftk::streaming_filter emitted, push() per input then finish(), in order);
arrays in numpy C order with the fastest axis last.  The woven series holds its 12 raw and 12 smoothed slices the same way.
No test runs this script or reads the reference; the weights also depend on the C library's exp of the machine it ran on."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# name: (dims fastest first, sigma, ksize, N, seed)
CASES = {
    "t2d_31x37_k1_n3": ((31, 37), 1.0, 1, 3, 21),
    "t2d_31x37_k3_n8": ((31, 37), 0.75, 3, 8, 22),
    "t2d_31x37_k5_n5": ((31, 37), 1.0, 5, 5, 23),
    "t2d_31x37_k5_n12": ((31, 37), 1.5, 5, 12, 24),
    "t2d_31x37_k7_n9": ((31, 37), 2.0, 7, 9, 25),
    "t2d_31x37_k9_n13": ((31, 37), 2.5, 9, 13, 26),
    # series shorter than the kernel: the reference emits 3, 1, 0, 3 arrays
    "t2d_31x37_k5_n4": ((31, 37), 1.0, 5, 4, 27),
    "t2d_31x37_k5_n3": ((31, 37), 1.0, 5, 3, 28),
    "t2d_31x37_k5_n2": ((31, 37), 1.0, 5, 2, 29),
    "t2d_31x37_k9_n6": ((31, 37), 2.0, 9, 6, 30),
    "tvec_2x6x5_k3_n6": ((2, 6, 5), 1.0, 3, 6, 31),
    "t3d_7x5x4_k5_n9": ((7, 5, 4), 1.25, 5, 9, 32),
}
EXPECTED_OUTPUTS = {"t2d_31x37_k5_n4": 3, "t2d_31x37_k5_n3": 1, "t2d_31x37_k5_n2": 0, "t2d_31x37_k9_n6": 3}


def random_input(dims, n, seed):
    """n seeded arrays of doubles in [-1, 1); one entry in 16 scaled by 1e-9, one in 32 a zero of either sign"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=(n,) + tuple(reversed(dims)))
    pick = rng.integers(0, 32, size=a.shape)
    a[pick < 2] *= 1e-9
    a[pick == 2] = 0.0
    a[pick == 3] = -0.0
    return a


def build_driver(ref, work):
    subprocess.check_call(["cmake", "-DREF=" + ref, "-DOUT=" + work, "-P", os.path.join(ROOT, "oracle", "gen_config.cmake")])
    exe = os.path.join(work, "temporal_driver")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-w", "-I" + os.path.join(ref, "include"), "-I" + os.path.join(work, "include"), "-o", exe,
                           os.path.join(HERE, "temporal_driver.cpp"), "-lpthread"])
    return exe


def reference_filter(exe, work, series, sigma, ksize):
    """series: (N, ...) raw arrays -> (weights, (n_emitted, ...) arrays)"""
    dims = list(reversed(series.shape[1:]))
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        np.array([ksize, series.shape[0], len(dims)] + dims, dtype=np.int64).tofile(f)
        np.array([sigma], dtype=np.float64).tofile(f)
        np.ascontiguousarray(series, dtype=np.float64).tofile(f)
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        ne = int(np.fromfile(f, dtype=np.int64, count=1)[0])
        w = np.fromfile(f, dtype=np.float64, count=ksize)
        out = np.fromfile(f, dtype=np.float64, count=ne * series[0].size).reshape((ne,) + series.shape[1:])
    return w, out


def main():
    import pyoracle
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with tempfile.TemporaryDirectory() as work:
        exe = build_driver(ref, work)
        for name, (dims, sigma, ksize, n, seed) in CASES.items():
            a = random_input(dims, n, seed)
            w, out = reference_filter(exe, work, a, sigma, ksize)
            assert name not in EXPECTED_OUTPUTS or len(out) == EXPECTED_OUTPUTS[name], (name, len(out))
            np.savez_compressed(os.path.join(HERE, name + ".npz"), dims=np.array(dims), sigma=sigma, ksize=ksize, input=a, weights=w, output=out)
            print(name, "emitted", len(out))
        # the end-to-end series: woven 31 x 37 x 12 plus seeded noise of amplitude 0.05, raw and smoothed (sigma 1, ksize 5)
        dims, DT, sigma, ksize = (31, 37), 12, 1.0, 5
        rng = np.random.default_rng(33)
        raw = np.stack([pyoracle.synthetic("woven", dims, k, DT) + rng.uniform(-0.05, 0.05, size=(dims[1], dims[0])) for k in range(DT)])
        w, sm = reference_filter(exe, work, raw, sigma, ksize)
        assert len(sm) == DT
        np.savez_compressed(os.path.join(HERE, "series_woven_noisy_31x37x12_k5.npz"), nd=2, dims=np.array(dims), DT=DT, sigma=sigma, ksize=ksize, raw=raw, weights=w, smoothed=sm)


if __name__ == "__main__":
    main()
