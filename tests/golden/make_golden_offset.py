#!/usr/bin/env python3
"""Generates tests/golden/offset/*.npz: the REAL reference (oracle/_ref/ftk_ref_driver) on arrays whose lattice does not begin at the
origin -- FTK_REF_ARRAY_START shifts set_array_domain and set_domain alike (oracle/ref_driver.cpp), the reference subtracts
local_array_domain.start(d) at every field access (2d:552-578, 3d:389-418) and in REGULAR_COORDS_BOUNDS (2d:504-510, 3d:358-365).
The scalar inputs are those of random_2d_scalar_29x24x6 and random_3d_scalar_13x12x11x4; the vector inputs are made here, values on a
1/64 grid.  Each start runs once with the lattice integers as coordinates and once with an image box.  The fixtures lie in a folder
of their own: common.golden_names() lists tests/golden/*.npz for the tests that sweep a fixture at the origin.  Build container only:

    make -C oracle ref && python tests/golden/make_golden_offset.py"""
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from refdump import read_dump  # noqa: E402

START = {2: (5, 7), 3: (5, 7, 3)}
BOUNDS = {2: [-1.5, 2.25, 10.0, 11.5], 3: [0.0, 1.0, -2.0, 2.0, 100.0, 130.0]}


def inputs():
    src2 = np.load(os.path.join(HERE, "random_2d_scalar_29x24x6.npz"))
    src3 = np.load(os.path.join(HERE, "random_3d_scalar_13x12x11x4.npz"))
    rng = np.random.default_rng(20261021)
    v2 = [rng.integers(-96, 97, size=(14, 17, 2)) / 64.0 for _ in range(4)]
    v3 = [rng.integers(-96, 97, size=(7, 8, 9, 3)) / 64.0 for _ in range(3)]
    return [("random_2d_scalar_29x24x6", [np.array(s) for s in src2["steps"]], 2, 1),
            ("random_3d_scalar_13x12x11x4", [np.array(s) for s in src3["steps"]], 3, 1),
            ("grid64_2d_vector_17x14x4", v2, 2, 2),
            ("grid64_3d_vector_9x8x7x3", v3, 3, 3)]


def main():
    if not os.path.exists(mg.DRIVER):
        sys.exit("build the reference driver first: make -C oracle ref")
    os.makedirs(os.path.join(HERE, "offset"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "o.bin")
        for name, steps, nd, nv in inputs():
            start = ",".join(str(v) for v in START[nd])
            for suffix, env, extra in (("", {}, {}), ("_bounds", {"FTK_REF_BOUNDS": ",".join(repr(b) for b in BOUNDS[nd])}, dict(bounds=np.array(BOUNDS[nd])))):
                mg.run_file(out, steps, nd, nv, env=dict(env, FTK_REF_ARRAY_START=start))
                d = read_dump(out)
                d["curves"] = d["pp"] = None                  # (pass 2 is not what these fixtures are for)
                mg.save(os.path.join("offset", name + "_at_" + "_".join(str(v) for v in START[nd]) + suffix), d,
                        dict(extra, array_start=np.array(START[nd])))


if __name__ == "__main__":
    main()
