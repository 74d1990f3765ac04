#!/usr/bin/env python3
"""Records what the REAL reference CPU path (oracle/_ref/ftk_ref_driver) returns on the seeded random series of
tests/test_oracle_fuzz_reference.py -> tests/golden/fuzz_reference.json.  Run in the build container only:

    make -C oracle ref && python tests/golden/make_golden_fuzz.py

The records of these series (noise fields: up to 10^5 records per series) would be megabytes, so each case keeps its record count, its
quantisation factors and the SHA-256 of its records in the canonical form tests/common.py::records_digest gives them -- what
assert_records_equal(..., coord_tol=0.0) compares, bit for bit."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import records_digest  # noqa: E402
from refdump import read_dump, write_input  # noqa: E402
from test_oracle_fuzz_reference import SEEDS, fuzz_cases  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "ftk_ref_driver")


def main():
    if not os.path.exists(DRIVER):
        sys.exit("build the reference driver first: make -C oracle ref")
    out = {}
    for seed in SEEDS:
        cases = []
        for steps, nd, nv, env, _opts, _what in fuzz_cases(seed):
            with tempfile.TemporaryDirectory() as tmp:
                inp, dump = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
                write_input(inp, steps, nd, nv)
                subprocess.run([DRIVER, "file", inp, dump, "8"], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                               env=dict(os.environ, **env), timeout=300)
                ref = read_dump(dump)
            cases.append({"records": int(len(ref["records"])), "factors": [int(f) for f in ref["factors"]],
                          "records_sha256": records_digest(ref["records"])})
        out[str(seed)] = cases
        print(seed, [c["records"] for c in cases])
    with open(os.path.join(HERE, "fuzz_reference.json"), "w") as f:
        json.dump({"made_by": "oracle/_ref/ftk_ref_driver file mode, tests/golden/make_golden_fuzz.py", "seeds": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
