"""The sets of tests/post_process_border_cases.py are what they claim to be -- checked WITHOUT a GPU, on the host function
ftkx_post_process_curves: the sizes and layouts, the values, the kept counts, and on every set's host result every effect that the set
must show (the -0.0 / 0.0 tie in t among them).  tests/test_gpu_post_process_borders.py runs the kernels on exactly these sets."""
import numpy as np
import pytest

import post_process_border_cases as B
from post_process_border_cases import K, SPINE


@pytest.mark.parametrize("name", B.ALL)
def test_set_shows_what_it_must(name):
    recs, offs, indices, loop, host = B.case(name)
    assert B.shows_what_it_must(name, recs, offs, indices, loop, host), (name, B.effects(recs, offs, indices, loop, host))
    n = int(offs[-1] - offs[0])
    lens = np.diff(offs)
    flat = indices[offs[0]:offs[-1]]
    assert len(np.unique(flat)) == n and flat.min() >= 0 and flat.max() < len(recs)
    assert np.all(loop[lens < 3] == 0) and set(np.unique(loop)) <= {0, 1}
    assert set(np.unique(recs["t"][flat].view(np.uint64))) == set(B.T_VALUES.view(np.uint64))       # -0.0 and 0.0 both
    assert set(np.unique(recs["aux"][flat] >> 1)) == {0, 1, 2, 3}
    if name in B.KEPT:
        n0, _, M = B.KEPT[name]
        assert n > 4 * K and n > n0 and len(host.indices) == M
        return
    layout, size, _, variant = B.SETS[name]
    assert n == B.SIZES[size]
    ordinal, ty = recs["aux"][flat] & 1, recs["type"][flat]
    if variant == "one_type":
        assert np.all(ty == 2) and len(host.indices) == n and len(host) == len(lens) and np.array_equal(host.loop, loop)   # not split mode: loops stay loops
    elif variant == "zero_type":
        assert np.all(ty == 0) and len(host.indices) == n and len(host) == len(lens) and not host.loop[lens > 0].any()      # split mode: no piece is a loop
    else:
        assert set(np.unique(ty)) == set(B.TYPES.tolist())
    assert ordinal.any() == (variant != "no_ordinal") and (not ordinal.all()) == (variant != "all_ordinal")
    heads = offs[:-1][lens > 0] - offs[0]
    if layout == "a":
        assert len(lens) == 1
    elif layout == "b":
        for L in (8, 512, 2048):
            assert np.any(lens == L) and np.all((offs[:-1][lens == L] % L) == 0)
        assert np.all(np.isin(lens[:-1], (8, 512, 2048))) and np.all(ordinal[::512] == 1)
    elif layout in ("c", "e"):
        assert 4 < lens[lens > 0].mean() < 6 and np.mean(lens == 1) > 0.15 and 0.05 < np.mean(lens == 0) < 0.15
    elif layout == "d-head":
        assert SPINE in heads
    elif layout == "d-straddle":
        c = int(np.searchsorted(offs, SPINE, side="right")) - 1
        assert offs[c] <= SPINE - 4096 and (offs[c + 1] >= SPINE + 4096 if size == "259K+1" else offs[c + 1] == n)
    if layout == "e":
        assert offs[0] == 1000 and len(recs) == 2 * n and np.all(indices[:1000] == -1)
    else:
        assert offs[0] == 0 and len(recs) == n


def test_every_size_and_layout_is_there():
    """the issue's table: (a) at every size, every layout at 256K + 1, (b) at 4K and 8K + 1, (c) at 4K + 1 and 257K + 1, (d) at 257K + 1,
    (e) at 8K + 1; the variants; the three kept counts"""
    have = {(s[0], s[1]) for s in B.SETS.values() if s[3] == "mixed"}
    for size in ("K-1", "K", "K+1", "4K-1", "4K", "4K+1", "8K+1", "256K", "256K+1", "257K+1"):
        assert ("a", size) in have
    for pair in [("b", "4K"), ("b", "8K+1"), ("c", "4K+1"), ("c", "257K+1"), ("d-head", "257K+1"), ("d-straddle", "257K+1"), ("d-straddle", "259K+1"), ("e", "8K+1"),
                 ("b", "256K+1"), ("c", "256K+1"), ("d-head", "256K+1"), ("e", "256K+1")]:
        assert pair in have
    assert {s[3] for s in B.SETS.values()} == {"mixed", "one_type", "zero_type", "no_ordinal", "all_ordinal"}
    assert {s[2] for s in B.SETS.values()} == {1.3, 4, 30}
    assert sorted(v[2] for v in B.KEPT.values()) == [4 * K, 4 * K + 1, 6 * K]
