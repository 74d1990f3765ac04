"""The mask kernels' launch plan (ftk_amd/csrc/mask_plan.hpp) computed WITHOUT a GPU: which kernel family takes which mesh, with what grid,
placement word, pieces of planes and summary geometry.  launch_masks launches what plan_masks returns, and march2_supported /
masks_have_summary / mask_summary_rows -- what the cull, the halo and the buffer sizes go by -- read the same plan; here the function is
driven through tests/hostcheck: the family table of the shapes the project talks about, the plan's own consistency over random shapes and
hook settings, and the complete plans of tests/golden/mask_plans.txt, which were printed by the launch code as it stood before the plan
was a function of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MARCH6, MARCH4, ROWS2, REDUCE, VEC2, VEC, GENERIC = range(7)
FIELDS = ("family", "march2", "has_summary", "u_rows", "gx", "gy", "gz", "block", "lds_bytes", "swizzle", "zchunk", "groups", "njobs", "npieces")


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_plan.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "hostcheck.cpp")])
    L = C.CDLL(so)
    L.hc_mask_plan.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_char_p]
    L.hc_mask_plan.restype = None
    return L


def plan(L, nd, scalar, dims, njobs=1, reduce=False, hooks=None, u_rows=None, pitch=None):
    d = list(dims) + [1] * (3 - len(dims))
    shape = (C.c_int * 6)(nd, int(scalar), d[0], d[1], d[2], pitch if pitch is not None else (d[0] + 7) // 8 * 8 + 8)
    out = (C.c_longlong * (14 + 2 * 47))()
    name = C.create_string_buffer(64)
    L.hc_mask_plan(shape, None if hooks is None else hooks.encode(), None if u_rows is None else str(u_rows).encode(), njobs, int(reduce), out, name)
    p = dict(zip(FIELDS, out[:14]))
    p["name"] = name.value.decode()
    p["pieces"] = [(out[14 + 2 * i], out[15 + 2 * i]) for i in range(p["npieces"])]
    return p


def test_family_table(hc):
    """Today's table.  The last eight rows are the shapes the fast kernels do not take (odd rows, rows that are no multiple of 8, slices of
    4 GiB and more, vector slices of 2 GiB and more, the reference's own test grids): work on shape generality shows as an edit here."""
    table = [
        # the five BASELINE configurations
        (2, True, (128, 128), MARCH4, "ftkx::mask_march4_kernel<2, false, 1, 8>", 4),
        (2, True, (1024, 1024), MARCH4, "ftkx::mask_march4_kernel<2, false, 1, 8>", 4),
        (3, True, (256, 256, 256), MARCH6, "ftkx::mask_march6_kernel<2, 4, 4, false>", 16),
        (3, True, (512, 512, 512), MARCH6, "ftkx::mask_march6_kernel<2, 4, 4, false>", 16),
        (2, False, (2048, 1024), VEC2, "ftkx::mask_vec2_kernel<2>", 4),
        # rows of 32 KB; two cases of test_mask_kernel_generations_agree (258: even, but no whole words of 8 -- no summaries)
        (2, True, (4096, 4096), ROWS2, "ftkx::mask_rows2_kernel<8>", 4),
        (2, True, (1024, 512), MARCH4, "ftkx::mask_march4_kernel<2, false, 1, 8>", 4),
        (2, True, (258, 100), MARCH4, "ftkx::mask_march4_kernel<2, false, 1, 8>", 0),
        # the hard ones
        (3, True, (513, 511, 509), GENERIC, "ftkx::mask_kernel<3>", 0),
        (2, True, (1025, 1023), GENERIC, "ftkx::mask_kernel<2>", 0),
        (2, True, (517, 515), GENERIC, "ftkx::mask_kernel<2>", 0),
        (3, True, (1024, 1024, 520), GENERIC, "ftkx::mask_kernel<3>", 0),
        (3, True, (1024, 1024, 1024), GENERIC, "ftkx::mask_kernel<3>", 0),
        (3, False, (512, 512, 512), VEC, "ftkx::mask_vec_kernel<3>", 1),
        (2, True, (31, 37), GENERIC, "ftkx::mask_kernel<2>", 0),
        (3, True, (31, 29, 37), GENERIC, "ftkx::mask_kernel<3>", 0),
        (2, False, (31, 37), GENERIC, "ftkx::mask_kernel<2>", 0),
        (3, False, (31, 29, 37), GENERIC, "ftkx::mask_kernel<3>", 0),
    ]
    for nd, scalar, dims, family, name, rows in table:          # rows: what a summary byte stands for, 0 = no summaries
        p = plan(hc, nd, scalar, dims, njobs=4)
        assert (p["family"], p["name"]) == (family, name), (dims, p)
        assert (p["has_summary"], p["u_rows"]) == (int(rows > 0), max(rows, 1)), (dims, p)
        assert p["march2"] == int(family in (MARCH6, MARCH4, ROWS2)), (dims, p)


def test_plan_is_consistent_over_random_shapes_and_hooks(hc):
    rng = np.random.default_rng(20261016)
    sizes = [1, 2, 3, 7, 8, 16, 31, 64, 100, 128, 130, 255, 256, 258, 264, 512, 520, 1024, 1030, 2048, 4096]
    knobs = {"swizzle": [0, 1, 8, 9, 16, 24, 25], "yg": [-1, 0, 1, 3, 4, 16, 255, 1000], "zchunk": [0, 1, 5, 7, 32, 100], "lmin": [0, 1, 6, 30], "lcap": [0, 1, 3, 24, 100000],
             "order": [0, 1], "rows": [-3, 0, 1, 2, 5, 64, 100], "lean": [0, 1]}
    seen = set()
    for it in range(4000):
        nd = int(rng.integers(2, 4))
        scalar = bool(rng.integers(0, 2))
        dims = [int(rng.choice(sizes)) if rng.random() < 0.7 else int(rng.integers(1, 1200)) for _ in range(nd)]
        hooks = ",".join("%s=%d" % (k, rng.choice(v)) for k, v in knobs.items() if rng.random() < 0.25) or None
        u = [None, None, -1, 0, 1, 4, 16][int(rng.integers(0, 7))]
        njobs = int(rng.integers(1, 40))
        DW, DH, DD = dims[0], dims[1], dims[2] if nd == 3 else 1
        normal = plan(hc, nd, scalar, dims, njobs=njobs, hooks=hooks, u_rows=u)
        pre = plan(hc, nd, scalar, dims, njobs=njobs, reduce=True, hooks=hooks, u_rows=u)
        what = (nd, scalar, dims, hooks, u, njobs, normal)
        fam = normal["family"]
        seen.add(fam)
        # summaries: exactly where the chosen family writes them (the marching kernels on rows of whole words, both vector kernels), unless switched off
        writes = fam in (VEC2, VEC) or (fam in (MARCH6, MARCH4, ROWS2) and DW % 8 == 0)
        assert normal["has_summary"] == int(writes and (u is None or u >= 0)), what
        geometry = {MARCH6: 4 if u == 4 else 16, MARCH4: 4, ROWS2: 4, VEC2: 4, VEC: 1, GENERIC: 1}[fam]
        assert normal["u_rows"] in (1, 4, 16) and normal["u_rows"] == (1 if not normal["has_summary"] or u == 1 else geometry), what
        assert (fam == VEC2) == (not scalar and normal["u_rows"] == 4), what
        # what the rest of the library asks does not depend on the launch it asks about
        assert all(pre[k] == normal[k] for k in ("march2", "has_summary", "u_rows")), (what, pre)
        # the pre-pass exists exactly where the marching kernels can walk the mesh
        assert (pre["family"] == REDUCE) == bool(pre["march2"]) and fam != REDUCE, (what, pre)
        assert bool(normal["march2"]) == (fam in (MARCH6, MARCH4, ROWS2)), what
        assert (fam == MARCH6) == bool(normal["march2"] and nd == 3) and (fam in (VEC2, VEC)) == (not scalar and DW >= 8 and DW % 8 == 0), what
        for p in (normal, pre):
            assert min(p["gx"], p["gy"], p["gz"]) >= 1 and p["block"] in (256,) and 0 <= p["lds_bytes"] <= 160 * 1024, (what, p)
            if p["family"] in (MARCH6, MARCH4, ROWS2, REDUCE) and p["swizzle"] & 8:
                yg = (p["swizzle"] >> 8) & 0xff
                assert yg >= 1 and p["gy"] % yg == 0, (what, p)
            # the pieces of a tile column: disjoint, covering [0, DD), at most 47, longest first
            if p["family"] == MARCH6:
                assert 1 <= p["npieces"] <= 47 and p["gz"] == p["npieces"] * njobs and abs(p["njobs"]) == njobs, (what, p)
                z = 0
                for z0, ln in p["pieces"]:
                    assert z0 == z and ln >= 1, (what, p)
                    z += ln
                assert z == DD, (what, p)
                lens = [ln for _, ln in p["pieces"]]
                assert lens == sorted(lens, reverse=True), (what, p)
            else:
                assert p["npieces"] == 0 and p["njobs"] == njobs, (what, p)
    assert seen == {MARCH6, MARCH4, ROWS2, VEC2, VEC, GENERIC}


def test_pinned_plans_of_the_launch_code_before_the_plan(hc):
    """every field of every entry of tests/golden/mask_plans.txt: the variants of test_mask_kernel_generations_agree on its shapes, the shapes of
    the family table with their pre-pass, hook values at their edges"""
    n = 0
    for line in open(os.path.join(HERE, "golden", "mask_plans.txt")):
        if line.startswith("#"):
            continue
        shape, hooks, u, name, fields, pieces = line.rstrip("\n").split("\t")
        nd, scalar, dw, dh, dd, pitch, njobs, reduce = (int(v) for v in shape.split())
        p = plan(hc, nd, scalar, (dw, dh, dd), njobs=njobs, reduce=bool(reduce), hooks=None if hooks == "-" else hooks, u_rows=None if u == "-" else u, pitch=pitch)
        assert p["name"] == name, (line, p)
        assert [p[k] for k in FIELDS] == [int(v) for v in fields.split()], (line, p)
        assert p["pieces"] == ([] if pieces == "-" else [tuple(int(v) for v in e.split(":")) for e in pieces.split(",")]), (line, p)
        n += 1
    assert n == 260
