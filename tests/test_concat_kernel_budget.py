"""The concat kernels at compile time (the method of tests/test_f32_kernel_budget.py: the compiler's kernel-resource-usage remarks for the
flags of the build).  They are pure streaming kernels: all four instantiations (float and double planes, 2 and 3 components), on both
paths (the 16-byte body and vertex by vertex), have no scratch.  LDS: none on the vertex-wise path and in the direct form of the body, which
double planes take; the body of float planes stages a workgroup's tile through LDS, and takes exactly the bytes concat_steps.hpp states."""
import os
import re

import pytest

from test_f32_kernel_budget import HIPCC, ROOT, resources


def stated(name):
    txt = open(os.path.join(ROOT, "ftk_amd", "csrc", "concat_steps.hpp")).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, txt)
    assert m, "concat_steps.hpp no longer states " + name
    return int(m.group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_concat_kernels_have_no_scratch_and_the_stated_lds(tmp_path):
    rows = resources("concat_kernels.hip", tmp_path)
    threads = stated("kConcatThreads")
    assert stated("kConcatLdsBytesDouble") == 0
    want = {}
    for nc in (2, 3):
        want["ftkx::concat_kernel_staged<float, %d>" % nc] = stated("kConcatLdsBytesFloat%d" % nc)
        assert want["ftkx::concat_kernel_staged<float, %d>" % nc] == threads * nc * 4 * 8          # a tile: every lane's nc * 4 doubles
        want["ftkx::concat_kernel<float, %d, false>" % nc] = 0
        want["ftkx::concat_kernel<double, %d, true>" % nc] = 0
        want["ftkx::concat_kernel<double, %d, false>" % nc] = 0
    assert sorted(k for k in rows if "concat_kernel" in k) == sorted(want), sorted(rows)              # these eight and no other
    for k, lds in want.items():
        assert int(rows[k]["ScratchSize [bytes/lane]"]) == 0, (k, rows[k])
        assert int(rows[k]["LDS Size [bytes/block]"]) == lds, (k, rows[k])
