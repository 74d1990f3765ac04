"""The series pass's sample kernel at compile time (the method of tests/test_sample_kernel_budget.py: the compiler's kernel-resource-usage
remarks for the flags of the build).  Both instantiations: no scratch, no LDS, no spills; at most 168 VGPRs -- the register rule of a split
pass's tail (a wavefront of it must fit next to two of the mask kernel's three per SIMD) --; and the occupancy NOTES.md
records for each instantiation (the table under "Series pass samples its own records") as the floor."""
import os
import re

import pytest

from test_f32_kernel_budget import HIPCC, ROOT, resources

TAIL_VGPRS = 168


def noted():
    """{nd: (VGPRs, waves per SIMD)} from the rows `| series_sample_kernel<nd> | VGPRs | SGPRs | waves/SIMD |` of NOTES.md"""
    txt = open(os.path.join(ROOT, "NOTES.md")).read()
    return {int(m.group(1)): (int(m.group(2)), int(m.group(4)))
            for m in re.finditer(r"\|\s*`?series_sample_kernel<(\d)>`?\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", txt)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_series_sample_kernels_fit_a_split_tail_and_keep_the_noted_occupancy(tmp_path):
    rows = resources("sample_kernels.hip", tmp_path)
    floor = noted()
    assert set(floor) == {2, 3}, "NOTES.md must record VGPRs, SGPRs and waves/SIMD of series_sample_kernel<2> and series_sample_kernel<3>"
    for nd in (2, 3):
        k = "ftkx::series_sample_kernel<%d>" % nd
        assert k in rows, (k, sorted(rows))
        print(k, rows[k])
        assert int(rows[k]["ScratchSize [bytes/lane]"]) == 0, (k, rows[k])
        assert int(rows[k]["LDS Size [bytes/block]"]) == 0, (k, rows[k])
        assert int(rows[k]["VGPRs Spill"]) == 0 and int(rows[k]["SGPRs Spill"]) == 0, (k, rows[k])
        assert int(rows[k]["VGPRs"]) <= TAIL_VGPRS, (k, rows[k])
        assert int(rows[k]["Occupancy [waves/SIMD]"]) >= floor[nd][1], (k, rows[k], floor[nd])
