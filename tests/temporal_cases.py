"""Temporal Gaussian smoothing: the reference's filter restated in numpy and the fixtures of tests/golden/temporal/.

Rules (include/ftk/filters/streaming_filter.hh and gaussian_kernel, include/ftk/ndarray/conv.hh:50-72, of the reference;
tests/golden/temporal/*.npz hold what its own code gives).  K = kernel size (odd), H = (K + 1) // 2, `data` a deque:
  weights  c = (K - 1) * 0.5, s = 2 * sigma * sigma, w[i] = exp(-(i - c) ** 2 / s); every weight divided by the sum taken in index order
  push(a)  data.append(a); if len(data) > K: data.popleft(), cursor -= 1
           if len(data) >= H: emit sum_i w[i] * data[max(0, i + cursor - H + 1)], cursor += 1
  finish   loop: data.popleft(); if len(data) >= H: emit sum_i w[i] * data[min(len(data) - 1, i)], cursor -= 1; else stop
  sum      the accumulator starts as the rounded product w[0] * x0; then per tap a rounded multiply and a rounded add, in order"""
import collections
import glob
import math
import os

import numpy as np

from conv_cases import random_input, same_bits      # noqa: F401  (same_bits: NaN positions agree, everything else bit for bit)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal")
KSIZES = (1, 3, 5, 7, 9)
SERIES = "series_woven_noisy_31x37x12_k5"
VECTOR = "tvec_2x6x5_k3_n6"
EXPECTED_OUTPUTS = {"t2d_31x37_k1_n3": 3, "t2d_31x37_k3_n8": 8, "t2d_31x37_k5_n5": 5, "t2d_31x37_k5_n12": 12, "t2d_31x37_k7_n9": 9, "t2d_31x37_k9_n13": 13,
                    "t2d_31x37_k5_n4": 3, "t2d_31x37_k5_n3": 1, "t2d_31x37_k5_n2": 0, "t2d_31x37_k9_n6": 3, "tvec_2x6x5_k3_n6": 6, "t3d_7x5x4_k5_n9": 9}


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "t*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def series():
    return load(SERIES)


def gaussian_weights(sigma, ksize):
    c = float(ksize - 1) * 0.5
    s = 2.0 * sigma * sigma
    w = np.zeros(ksize)
    total = 0.0
    for i in range(ksize):
        x = float(i) - c
        w[i] = math.exp(-(x * x) / s)
        total += w[i]
    return w / total


def combine(arrays, weights):
    """one emission: whole-array products and sums, tap by tap"""
    with np.errstate(all="ignore"):
        acc = np.float64(weights[0]) * np.asarray(arrays[0], dtype=np.float64)
        for i in range(1, len(weights)):
            acc = acc + np.float64(weights[i]) * np.asarray(arrays[i], dtype=np.float64)
    return acc


class Filter:
    """the state machine; push() and finish_step() return the deque places the taps read (None: nothing emitted)"""

    def __init__(self, ksize):
        self.K, self.H = ksize, (ksize + 1) // 2
        self.data = collections.deque()
        self.cursor = 0

    def push(self, a):
        self.data.append(a)
        if len(self.data) > self.K:
            self.data.popleft(); self.cursor -= 1
        if len(self.data) < self.H:
            return None
        idx = [max(0, i + self.cursor - self.H + 1) for i in range(self.K)]
        self.cursor += 1
        return idx

    def finish_step(self):
        if not self.data:
            return None
        self.data.popleft()
        if len(self.data) < self.H:
            return None
        idx = [min(len(self.data) - 1, i) for i in range(self.K)]
        self.cursor -= 1
        return idx


def smooth_series(raw, weights, trace=None):
    """every array the filter emits for the raw series, in order; trace: takes ('push' | 'finish', idx or None) per step"""
    f = Filter(len(weights))
    out = []
    for a in raw:
        idx = f.push(a)
        if trace is not None:
            trace.append(("push", idx))
        if idx is not None:
            out.append(combine([f.data[j] for j in idx], weights))
    while len(raw):
        idx = f.finish_step()
        if trace is not None:
            trace.append(("finish", idx))
        if idx is None:
            break
        out.append(combine([f.data[j] for j in idx], weights))
    return out


def closed_form(raw, weights):
    """N >= K only: output n = sum_i w[i] * in[clamp(n + i - (H - 1), 0, N - 1)]"""
    K, N = len(weights), len(raw)
    H = (K + 1) // 2
    return [combine([raw[min(max(n + i - (H - 1), 0), N - 1)] for i in range(K)], weights) for n in range(N)]
