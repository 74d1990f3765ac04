"""The narrow input path at compile time (the method of tests/test_f32_kernel_budget.py: the compiler's kernel-resource-usage remarks for the
flags of the build, one compile of narrow_kernels.hip).  The narrow kernels are pure streaming kernels: every instantiation -- eight element
types, the 4-element body and the element-wise form -- has no scratch and no LDS, and few enough registers for 8 wavefronts per SIMD (the
most a SIMD of gfx950 holds: 512 VGPRs / 8 = 64 per lane)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
TYPES = ("ftkx::NarrowHalf", "ftkx::NarrowBf16", "unsigned char", "signed char", "unsigned short", "short", "unsigned int", "int")


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
def test_narrow_kernels_are_streaming_kernels(tmp_path):
    rows = resources("narrow_kernels.hip", tmp_path)
    kernels = [k for k in rows if k.startswith("ftkx::narrow_kernel<")]
    assert len(kernels) == 2 * len(TYPES), sorted(rows)
    for t in TYPES:
        for vec in ("true", "false"):
            k = "ftkx::narrow_kernel<%s, %s>" % (t, vec)
            assert k in rows, (k, sorted(rows))
            print(k, rows[k].get("VGPRs"), rows[k].get("SGPRs"), rows[k].get("Occupancy [waves/SIMD]"))
            assert int(rows[k]["ScratchSize [bytes/lane]"]) == 0, (k, rows[k])
            assert int(rows[k]["LDS Size [bytes/block]"]) == 0, (k, rows[k])
            assert int(rows[k]["VGPRs"]) + int(rows[k].get("AGPRs", 0)) <= 64, (k, rows[k])
            assert int(rows[k]["Occupancy [waves/SIMD]"]) == 8, (k, rows[k])
