"""The three orders in which mask_march6_kernel's workgroups take the (slice, piece) pairs of a launch (ZPlan, mask_plan.hpp: slice by
slice, piece by piece over all slices, slices in groups): the order is a renumbering of the same workgroups, so whichever one a launch
takes, the series gives the same records byte for byte, the same factors and the same cull statistics.  That the renumbering is one --
every pair exactly once -- is tests/test_mask_order.py's, without a GPU; here the kernel runs under it, on shapes with uneven groups,
partial tiles and many pieces."""
import os

import numpy as np
import pytest

from test_gpu_properties import _run

pytestmark = pytest.mark.gpu

VARIANTS = ["order=0", "order=1", "order=2,sgroup=1", "order=2,sgroup=2", "order=2,sgroup=3", "order=2,sgroup=100",
            "order=2,sgroup=2,lcap=3,lmin=1", "order=2,sgroup=2,swizzle=0"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


# 130 x 70 x 40, 5 slices: pieces of 18 / 9 / 7 / 6 planes, groups of 2 + 2 + 1 slices at sgroup=2, a partial tile in x and in y
@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("dims,nt", [((130, 70, 40), 5), ((256, 128, 72), 6)])
def test_every_order_of_the_workgroups_gives_the_same_series(gpu, dims, nt, rough):
    steps = None
    if rough:   # the seeded field of test_mask_kernel_generations_agree: plateaus, ties and noise -- mask words and block bytes are really stored
        rng = np.random.default_rng(7)
        shape = tuple(reversed(dims))
        steps = [np.round(rng.standard_normal(shape) * 2) * 0.25 + rng.integers(-2, 3, size=shape) / 64.0 for _ in range(nt)]
    first = None
    for plan in VARIANTS:
        old = os.environ.get("FTKX_MASK_PLAN")
        os.environ["FTKX_MASK_PLAN"] = plan
        try:
            recs, st, factors = _run(gpu, "moving_extremum_3d", dims, nt, steps=steps)
        finally:
            if old is None:
                os.environ.pop("FTKX_MASK_PLAN", None)
            else:
                os.environ["FTKX_MASK_PLAN"] = old
        got = (recs, tuple(factors), st["cells_survived"], st["simplices_tested"])
        if first is None:
            first = got
            assert st["cull_enabled"] == 1 and len(recs) > 0
            continue
        assert got[1:] == first[1:], (plan, got[1:], first[1:])
        assert len(recs) == len(first[0]) and np.array_equal(recs.view(np.uint8), first[0].view(np.uint8)), plan      # byte for byte
