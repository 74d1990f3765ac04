"""The adjust kernels at compile time (the method of tests/test_f32_kernel_budget.py: the compiler's kernel-resource-usage remarks for the flags
of the build).  No instantiation has scratch or LDS.  The clamp-only ones are streaming kernels and keep the full 8 wavefronts per SIMD.  The
perturbing ones carry a Philox call and two quantile evaluations per lane; their registers and occupancy are written down in NOTES.md
("Perturbation and clamp") and held here to no scratch and at least 4 wavefronts per SIMD."""
import os

import pytest

from test_f32_kernel_budget import HIPCC, resources

KERNELS = ["ftkx::adjust_kernel<%s, %s, %s>" % (t, p, c) for t in ("double", "float") for p, c in (("true", "true"), ("true", "false"), ("false", "true"))]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return resources("adjust_kernels.hip", tmp_path_factory.mktemp("adjust_budget"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_every_instantiation_is_there_without_scratch_or_lds(rows):
    for k in KERNELS:
        assert k in rows, (k, sorted(rows))
        assert int(rows[k]["ScratchSize [bytes/lane]"]) == 0, (k, rows[k])
        assert int(rows[k]["LDS Size [bytes/block]"]) == 0, (k, rows[k])
    assert not [k for k in rows if "adjust_kernel" in k and k not in KERNELS], sorted(rows)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_occupancy(rows):
    for k in KERNELS:
        print(k, "VGPRs", rows[k]["VGPRs"], "SGPRs", rows[k]["TotalSGPRs"], "waves/SIMD", rows[k]["Occupancy [waves/SIMD]"])
        clamp_only = "<double, false, true>" in k or "<float, false, true>" in k
        assert int(rows[k]["Occupancy [waves/SIMD]"]) >= (8 if clamp_only else 4), (k, rows[k])
