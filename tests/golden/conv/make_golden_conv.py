"""Regenerates tests/golden/conv/*.npz from the REAL reference: tests/golden/conv/conv_driver.cpp (this repository's text) is compiled in a
scratch directory against the reference's headers and a config.hh made by oracle/gen_config.cmake, and run once per case.

    python tests/golden/conv/make_golden_conv.py [REFERENCE_ROOT]

Every file holds: nd, dims (x first), sigma, ksize, input, weights (the reference's gaussian_kernel2D / 3D), output
(conv_gaussian(input, sigma, ksize, ksize // 2)); arrays in numpy C order with x last.  The woven series holds DT raw and DT smoothed slices.
No test runs this script or reads the reference; the weights also depend on the C library's exp of the machine it ran on."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# name: (dims x first, sigma, ksize, seed)
CASES = {
    "conv2d_31x37_k3": ((31, 37), 1.0, 3, 11),
    "conv2d_31x37_k5": ((31, 37), 1.5, 5, 12),
    "conv2d_6x5_k7": ((6, 5), 2.0, 7, 13),
    "conv3d_31x29x37_k3": ((31, 29, 37), 1.0, 3, 14),
    "conv3d_17x13x11_k5": ((17, 13, 11), 1.25, 5, 15),
    "conv3d_4x3x3_k7": ((4, 3, 3), 2.0, 7, 16),
    "conv3d_4x3x3_k9": ((4, 3, 3), 3.0, 9, 17),
}


def random_input(dims, seed):
    """seeded doubles in [-1, 1); one entry in 16 scaled by 1e-9, one in 32 a zero of either sign"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=tuple(reversed(dims)))
    pick = rng.integers(0, 32, size=a.shape)
    a[pick < 2] *= 1e-9
    a[pick == 2] = 0.0
    a[pick == 3] = -0.0
    return a


def build_driver(ref, work):
    subprocess.check_call(["cmake", "-DREF=" + ref, "-DOUT=" + work, "-P", os.path.join(ROOT, "oracle", "gen_config.cmake")])
    exe = os.path.join(work, "conv_driver")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-w", "-I" + os.path.join(ref, "include"), "-I" + os.path.join(work, "include"), "-o", exe,
                           os.path.join(HERE, "conv_driver.cpp"), "-lpthread"])
    return exe


def reference_conv(exe, work, a, sigma, ksize):
    nd = a.ndim
    dims = list(reversed(a.shape))
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        np.array([nd, ksize] + dims, dtype=np.int64).tofile(f)
        np.array([sigma], dtype=np.float64).tofile(f)
        np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        nout = [int(v) for v in np.fromfile(f, dtype=np.int64, count=nd)]
        assert nout == dims, (nout, dims)
        w = np.fromfile(f, dtype=np.float64, count=ksize ** nd).reshape((ksize,) * nd)
        out = np.fromfile(f, dtype=np.float64, count=a.size).reshape(a.shape)
    return w, out


def main():
    import pyoracle
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with tempfile.TemporaryDirectory() as work:
        exe = build_driver(ref, work)
        for name, (dims, sigma, ksize, seed) in CASES.items():
            a = random_input(dims, seed)
            w, out = reference_conv(exe, work, a, sigma, ksize)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), nd=len(dims), dims=np.array(dims), sigma=sigma, ksize=ksize, input=a, weights=w, output=out)
        # the end-to-end series: woven 31 x 37 x 8 plus seeded noise of amplitude 0.05, raw and smoothed (sigma 1, ksize 3)
        dims, DT, sigma, ksize = (31, 37), 8, 1.0, 3
        rng = np.random.default_rng(18)
        raw = np.stack([pyoracle.synthetic("woven", dims, k, DT) + rng.uniform(-0.05, 0.05, size=(dims[1], dims[0])) for k in range(DT)])
        sm = []
        for k in range(DT):
            w, out = reference_conv(exe, work, raw[k], sigma, ksize)
            sm.append(out)
        np.savez_compressed(os.path.join(HERE, "series_woven_noisy_31x37x8_k3.npz"), nd=2, dims=np.array(dims), DT=DT, sigma=sigma, ksize=ksize, raw=raw, weights=w,
                            smoothed=np.stack(sm))


if __name__ == "__main__":
    main()
