"""The sample kernel at compile time (the method of tests/test_f32_kernel_budget.py: the compiler's kernel-resource-usage remarks for the flags
of the build).  Both instantiations are there, without scratch and without LDS; registers are not fixed here -- the occupancy NOTES.md
records for each instantiation (the table under "Auxiliary scalar fields") is the floor the kernel is held to."""
import os
import re

import pytest

from test_f32_kernel_budget import HIPCC, ROOT, resources


def noted_occupancy():
    """{nd: waves per SIMD} from the rows `| sample_kernel<nd> | VGPRs | waves/SIMD |` of NOTES.md"""
    txt = open(os.path.join(ROOT, "NOTES.md")).read()
    return {int(m.group(1)): int(m.group(3)) for m in re.finditer(r"\|\s*`?sample_kernel<(\d)>`?\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", txt)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_sample_kernels_have_no_scratch_no_lds_and_the_noted_occupancy(tmp_path):
    rows = resources("sample_kernels.hip", tmp_path)
    floor = noted_occupancy()
    assert set(floor) == {2, 3}, "NOTES.md must record VGPRs and waves/SIMD of sample_kernel<2> and sample_kernel<3>"
    for nd in (2, 3):
        k = "ftkx::sample_kernel<%d>" % nd
        assert k in rows, (k, sorted(rows))
        print(k, rows[k])
        assert int(rows[k]["ScratchSize [bytes/lane]"]) == 0, (k, rows[k])
        assert int(rows[k]["LDS Size [bytes/block]"]) == 0, (k, rows[k])
        assert int(rows[k]["VGPRs Spill"]) == 0 and int(rows[k]["SGPRs Spill"]) == 0, (k, rows[k])
        assert int(rows[k]["Occupancy [waves/SIMD]"]) >= floor[nd], (k, rows[k], floor[nd])
