"""Spatial Gaussian smoothing: the reference's rules restated in numpy, the fixtures of tests/golden/conv/ and the shapes the GPU tests use.

Rules (include/ftk/ndarray/conv.hh of the reference; tests/golden/conv/*.npz hold what its own code gives):
  weights  c = (ksize - 1) * 0.5, s = 2 * sigma * sigma, w = exp(-r / s) with r = x*x + y*y (+ z*z) left to right; every weight divided by the
           sum, which grows in the reference's loop order -- 2D: y outer, x inner; 3D: y outer, then x, then z innermost
  conv     padding ksize // 2; res = +0.0; kz outer, ky, kx innermost; a tap inside the array adds data * w (product rounded, then the sum);
           taps outside are skipped; finally res / ksize ** nd
Arrays are numpy C order with x last, weights included."""
import glob
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv")
KSIZES = (1, 3, 5, 7, 9)


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "conv*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def series():
    return load("series_woven_noisy_31x37x8_k3")


def gaussian_weights(nd, sigma, ksize):
    c = float(ksize - 1) * 0.5
    s = 2.0 * sigma * sigma
    w = np.zeros((ksize,) * nd)
    total = 0.0
    for j in range(ksize):
        for i in range(ksize):
            for k in range(ksize if nd == 3 else 1):
                x, y, z = float(i) - c, float(j) - c, float(k) - c
                r = x * x + y * y + z * z if nd == 3 else x * x + y * y
                v = math.exp(-r / s)
                if nd == 3:
                    w[k, j, i] = v
                else:
                    w[j, i] = v
                total += v
    return w / total


def conv(data, weights):
    """one whole-array multiply and one whole-array add per tap, in the reference's tap order: every output sees its in-range taps in that order"""
    a = np.ascontiguousarray(data, dtype=np.float64)
    nd = a.ndim
    K = weights.shape[0]
    p = K // 2
    if nd == 2:
        a = a[None]
        weights = weights[None]
    D, H, W = a.shape
    res = np.zeros_like(a)

    def span(n, k):         # outputs o with 0 <= o - p + k < n
        lo, hi = max(0, p - k), min(n, n + p - k)
        return (lo, hi) if lo < hi else None

    for kz in range(K if nd == 3 else 1):
        sz = span(D, kz) if nd == 3 else (0, 1)
        for ky in range(K):
            sy = span(H, ky)
            for kx in range(K):
                sx = span(W, kx)
                if sz is None or sy is None or sx is None:
                    continue
                oz = 0 if nd == 2 else kz - p
                dst = res[sz[0]:sz[1], sy[0]:sy[1], sx[0]:sx[1]]
                src = a[sz[0] + oz:sz[1] + oz, sy[0] + ky - p:sy[1] + ky - p, sx[0] + kx - p:sx[1] + kx - p]
                with np.errstate(all="ignore"):
                    dst += src * weights[kz, ky, kx]
    with np.errstate(all="ignore"):
        res /= float(K ** nd)
    return res[0] if nd == 2 else res


def conv_with_zeros(data, weights):
    """the other admissible form: taps outside the array take part with the value +0.0"""
    a = np.ascontiguousarray(data, dtype=np.float64)
    K = weights.shape[0]
    p = K // 2
    padded = np.pad(a, p)
    res = np.zeros_like(a)
    idx = [range(K)] * a.ndim
    import itertools
    for ks in itertools.product(*idx):
        sl = tuple(slice(k, k + n) for k, n in zip(ks, a.shape))
        with np.errstate(all="ignore"):
            res += padded[sl] * weights[ks]
    with np.errstate(all="ignore"):
        res /= float(K ** a.ndim)
    return res


def same_bits(got, exp):
    """NaN positions agree; everything else bit for bit"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return False
    ng, ne = np.isnan(got), np.isnan(exp)
    return bool(np.array_equal(ng, ne) and np.array_equal(got.view(np.uint64)[~ng], exp.view(np.uint64)[~ne]))


def random_input(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=shape)
    pick = rng.integers(0, 32, size=a.shape)
    a[pick < 2] *= 1e-9
    a[pick == 2] = 0.0
    a[pick == 3] = -0.0
    return a


# ---- the GPU tests' shapes (x, y[, z]): either side of every tile edge of conv_kernels.hip -- 32 along x, 32 (2D) or 8 (3D) along y, 8 or
# 4 along z, all powers of two -- and arrays shorter than the kernel
_W2 = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
SHAPES_2D = list(dict.fromkeys([(w, h) for w in _W2 for h in (1, 2, 9)] + [(h, w) for w in _W2 for h in (1, 2, 9)]))
_X3 = (1, 2, 5, 31, 32, 33, 63, 64, 65, 129)
_YZ3 = (1, 2, 7, 8, 9, 15, 16, 17, 33)


def _shapes_3d():
    out = []
    for i, x in enumerate(_X3):
        for j in range(4):
            y = _YZ3[(2 * i + 3 * j) % 9]
            z = _YZ3[(5 * i + 2 * j + 4) % 9]
            out.append((x, y, z))
    return out


SHAPES_3D = _shapes_3d()
assert len(set(SHAPES_3D)) == 40 and all(x * y * z <= 200000 for x, y, z in SHAPES_3D)
assert {s[1] for s in SHAPES_3D} == set(_YZ3) and {s[2] for s in SHAPES_3D} == set(_YZ3)
INF_CASE_2D, NAN_CASE_2D = (33, 9), (9, 33)        # these two carry an in-range Inf / NaN
INF_CASE_3D, NAN_CASE_3D = SHAPES_3D[13], SHAPES_3D[22]


def shape_input(shape, ksize):
    """the input of one GPU border case (shape x first)"""
    a = random_input(tuple(reversed(shape)), 1000 * len(shape) + 7 * sum(shape) + ksize)
    special = {INF_CASE_2D: np.inf, NAN_CASE_2D: np.nan, INF_CASE_3D: -np.inf, NAN_CASE_3D: np.nan}.get(tuple(shape))
    if special is not None:
        a.flat[a.size // 3] = special
        if np.isinf(special):
            a.flat[a.size // 3 + 1] = -special        # (next to it: some outputs see Inf - Inf)
    return a
