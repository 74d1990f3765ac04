"""Spatial smoothing of vector arrays, every component as the scalar field it is: the rule restated over tests/conv_cases.py, and the cases
the host and the GPU tests share.

    conv_vec(V)[..., c] == conv(V[..., c])        (conv_cases.conv: the reference's conv2D / conv3D restated, pinned to its outputs)

Arrays are numpy C order with x last among the spatial axes and the component axis behind them."""
import numpy as np

import conv_cases as CC

# (x, y[, z]): either side of the tile edges of conv_steps.hpp (32 along x; 32 / 8 along y; 8 or 4 along z), arrays shorter than the kernel
SHAPES_2D = [(31, 37), (33, 32), (32, 33), (65, 2), (2, 3), (1, 1)]
SHAPES_3D = [(33, 9, 9), (32, 8, 8), (33, 9, 5), (2, 7, 1), (4, 3, 3)]
SPECIAL_2D, SPECIAL_3D = (33, 32), (33, 9, 5)          # these carry an in-range Inf in one component and a NaN in another
FACTORS = (1.0, 2.0, 0.5)                                # the fixtures' components: S, 2 S, S / 2 -- powers of two commute with every rounding


def conv_vec(V, w):
    """THE oracle: conv_cases.conv per component"""
    V = np.ascontiguousarray(V, dtype=np.float64)
    return np.stack([CC.conv(V[..., c], w) for c in range(V.shape[-1])], axis=-1)


def fixture_vector(f):
    """a fixture of tests/golden/conv/ as a vector case: (V, expected) with components (S, 2 S[, S / 2]) and outputs (O, 2 O[, O / 2])"""
    nd = int(f["nd"])
    V = np.stack([f["input"] * k for k in FACTORS[:nd]], axis=-1)
    O = np.stack([f["output"] * k for k in FACTORS[:nd]], axis=-1)
    return np.ascontiguousarray(V), np.ascontiguousarray(O)


def shape_vector(shape, ksize, f32=False):
    """the input of one border case (shape x first) -> (V, clean): V has nd components; where the shape is a special one, component 0 holds an
    Inf (and its opposite next to it) and component 1 a NaN, and `clean` is V without them (else clean is V)"""
    nd = len(shape)
    comps = [CC.random_input(tuple(reversed(shape)), 5000 * nd + 11 * sum(shape) + 3 * ksize + c) for c in range(nd)]
    clean = np.stack(comps, axis=-1)
    if f32:
        clean = clean.astype(np.float32).astype(np.float64)
    V = clean.copy()
    if tuple(shape) in (SPECIAL_2D, SPECIAL_3D):
        n = V[..., 0].size
        V[..., 0].flat[n // 3] = np.inf
        V[..., 0].flat[n // 3 + 1] = -np.inf
        V[..., 1].flat[n // 2] = np.nan
    return V, clean


def check_against_restatement(got, V, clean, w, what):
    """got == conv_vec(V) as bits; and where V carries Inf / NaN in components 0 and 1, every OTHER component equals its clean result"""
    exp = conv_vec(V, w)
    assert CC.same_bits(got, exp), what
    if V is not clean and not np.array_equal(V.view(np.uint64), clean.view(np.uint64)):
        cl = conv_vec(clean, w)
        assert not np.isfinite(got[..., 0]).all() and np.isnan(got[..., 1]).any(), what
        assert not np.isinf(got[..., 1]).any(), (what, "the Inf of component 0 reached component 1")
        for c in range(2, V.shape[-1]):
            assert np.array_equal(got[..., c].view(np.uint64), cl[..., c].view(np.uint64)), (what, c)
        # where neither special value reaches, components 0 and 1 are their clean results too
        for c in (0, 1):
            same = np.isfinite(got[..., c])
            assert same.any() and np.array_equal(got[..., c][same].view(np.uint64), cl[..., c][same].view(np.uint64)), (what, c)


def weights(nd, ksize):
    return CC.gaussian_weights(nd, 0.75 + 0.25 * ksize, ksize)
