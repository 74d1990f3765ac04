"""ftkx_trace_curves_device and ftkx_pass2_device on chains that take pointer jumping many launches (tests/trace_long_cases.py): one open
path and one closed curve of more than 20 000 records each, and the path cut into pieces of 1, 2, 3, 16, 17, 256, 257, 4 096 and 4 097
points -- the lengths at the chains' ends, the closed-curve rule and the scatter to seed +- hops, against the host trace; then both
halves of pass 2 on the device against both on the host.  tests/test_trace_long_cases.py asserts on the host what each set is."""
import numpy as np
import pytest

import trace_long_cases as T
from test_gpu_post_process_device import assert_same
from test_gpu_trace_device import assert_same_curves

pytestmark = pytest.mark.gpu
SETS = ["open", "closed", "cut"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    import ftk_amd
    assert torch.cuda.is_available()
    c = ftk_amd.Context(2)
    yield c
    c.close()


@pytest.mark.parametrize("name", SETS)
def test_trace(ctx, name):
    import ftk_amd
    recs = T.records(name)
    assert T.shows_what_it_must(name)
    host = T.host_curves(name)
    for rep in range(2):
        dev = ftk_amd.trace_curves(2, T.DOMAIN, recs, ctx=ctx, device=True)
        assert ctx.trace_last_path() == 2
        assert_same_curves(dev, host, "%s, call %d" % (name, rep))


@pytest.mark.parametrize("name", SETS)
def test_pass2(ctx, name):
    import ftk_amd
    recs = T.records(name)
    assert T.shows_what_it_must(name)
    c1, l1, n1, ts1, _a, _b = ftk_amd.pass2(2, T.DOMAIN, recs)
    assert_same_curves((c1, l1, n1), T.host_curves(name))
    c2, l2, n2, ts2, _a, _b = ftk_amd.pass2(2, T.DOMAIN, recs, ctx=ctx, device=True, post_device=True)
    assert ctx.trace_last_path() == 2 and ctx.post_process_last_path() == 2
    assert_same_curves((c2, l2, n2), (c1, l1, n1), name)
    assert_same(ts2, ts1, name)


def test_closed_curve_with_device_resident_tags(ctx):
    import torch
    import ftk_amd
    recs = T.records("closed")
    tags = torch.from_numpy(np.ascontiguousarray(recs["tag"]).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = ftk_amd.trace_curves(2, T.DOMAIN, None, ctx=ctx, device=True, tags=tags)
    assert ctx.trace_last_path() == 2
    assert_same_curves(dev, T.host_curves("closed"))
