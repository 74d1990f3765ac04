"""ftkx_post_process_curves_device at the borders of its scan (post_process_kernels.hip) against the host function: the sets of
tests/post_process_border_cases.py -- one tile and four tiles plus and minus one point, the switch from one workgroup with a carry to three
launches at 8 192 points, more than 256 tiles so that the spine runs a second batch with a carry, curves that start on a thread's, a
wave's, a tile's and a spine batch's first element, kept counts on a tile's border under a grid sized by more points, and -0.0 / 0.0 ties
in t everywhere.  tests/test_post_process_border_cases.py asserts on the host what each set shows."""
import pytest

import post_process_border_cases as B
from test_gpu_post_process_device import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    import ftk_amd
    assert torch.cuda.is_available()
    c = ftk_amd.Context(2)
    yield c
    c.close()


@pytest.mark.parametrize("name", B.ALL)
def test_border_sets(ctx, name):
    import ftk_amd
    recs, offs, indices, loop, host = B.case(name)
    assert B.shows_what_it_must(name, recs, offs, indices, loop, host)
    if name in B.KEPT:
        assert len(host.indices) == B.KEPT[name][2]
    dev = ftk_amd.post_process_curves(recs, offs, indices, loop, ctx=ctx, device=True)
    assert ctx.post_process_last_path() == 2
    assert_same(dev, host, name)


def test_buffers_grow_and_are_reused_by_smaller_calls():
    """one fresh context: 2K - 1 points (one workgroup), 257K + 1 (the buffers grow; three launches, two batches of the spine), the
    2K - 1 set again in the larger buffers (back to one workgroup), then 8K + 1 with offsets[0] = 1 000 and unused records"""
    import ftk_amd
    ctx = ftk_amd.Context(2)
    try:
        for name in ("a-2K-1", "c-257K+1", "a-2K-1", "e-8K+1"):
            recs, offs, indices, loop, host = B.case(name)
            dev = ftk_amd.post_process_curves(recs, offs, indices, loop, ctx=ctx, device=True)
            assert ctx.post_process_last_path() == 2
            assert_same(dev, host, name)
    finally:
        ctx.close()
