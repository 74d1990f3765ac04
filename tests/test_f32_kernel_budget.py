"""The float32 input path at compile time (the method of tests/test_kernel_budget.py: the compiler's kernel-resource-usage remarks for the
flags of the build).  The widen kernels are pure streaming kernels and have no scratch; templating the convolution on its source type must
cost it nothing: every float-source instantiation has no scratch, the LDS of its FP64 counterpart and at least that one's occupancy --
the counterpart compiled in the same run, not a number written down here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def resources(name, tmp_path):
    """{demangled kernel: {remark: value}} of ftk_amd/csrc/<name>"""
    src = os.path.join(ROOT, "ftk_amd", "csrc", name)
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", src, "-o", str(tmp_path / (name + ".o")),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(\w[\w \[\]/]*): +(\S+)", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", cur).replace("void ", "")
            rows[cur] = {}
        elif cur:
            rows[cur][k] = v
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_widen_kernels_have_no_scratch(tmp_path):
    rows = resources("widen_kernels.hip", tmp_path)
    for k in ("ftkx::widen_kernel<true>", "ftkx::widen_kernel<false>"):
        assert k in rows, (k, sorted(rows))
        assert int(rows[k]["ScratchSize [bytes/lane]"]) == 0, (k, rows[k])
        assert int(rows[k]["LDS Size [bytes/block]"]) == 0, (k, rows[k])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_float_source_convolution_costs_what_its_fp64_counterpart_costs(tmp_path):
    rows = resources("conv_kernels.hip", tmp_path)
    for nd in (2, 3):
        for k in (1, 3, 5, 7, 9):
            f, d = "ftkx::conv_kernel<%d, %d, float>" % (nd, k), "ftkx::conv_kernel<%d, %d, double>" % (nd, k)
            assert f in rows and d in rows, (f, d, sorted(rows))
            assert int(rows[f]["ScratchSize [bytes/lane]"]) == 0, (f, rows[f])
            assert int(rows[f]["LDS Size [bytes/block]"]) == int(rows[d]["LDS Size [bytes/block]"]), (f, rows[f], rows[d])
            assert int(rows[f]["Occupancy [waves/SIMD]"]) >= int(rows[d]["Occupancy [waves/SIMD]"]), (f, rows[f], rows[d])
