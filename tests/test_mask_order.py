"""The order in which mask_march6_kernel's workgroups take the (slice, piece) pairs of a launch (ftk_amd/csrc/mask_plan.hpp: ZPlan,
zplan_decode), checked WITHOUT a GPU: the kernel and this test call the same decode, compiled here for the host.  Over blockIdx.z =
0 .. grid[2] - 1 every (job, piece) pair is taken exactly once in each of the three orders; the two older orders are the formulas the
kernel carried before the decode was a function of its own; in the third the slices go in groups that are as even as possible, piece by
piece inside a group; and the plan picks that order exactly where it says it does."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MARCH6 = 0
CAP = 47 * 64


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck") / "libhostcheck_order.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "mask_order.cpp")])
    L = C.CDLL(so)
    L.hc_mask_order.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_uint), C.c_uint]
    L.hc_mask_order.restype = None
    return L


def order_of(L, dims, njobs, hooks=None):
    """-> the plan's (family, gz, njobs, npieces, sgroup) and the (job, piece) of every blockIdx.z (None: not the 3D marching kernel)"""
    shape = (C.c_int * 6)(3, 1, dims[0], dims[1], dims[2], (dims[0] + 7) // 8 * 8 + 8)
    head = (C.c_longlong * 6)()
    where = (C.c_uint * (2 * CAP))()
    L.hc_mask_order(shape, None if hooks is None else hooks.encode(), njobs, head, where, CAP)
    p = dict(zip(("family", "gz", "njobs", "npieces", "sgroup"), head[:5]))
    if p["family"] != MARCH6:
        return p, None
    assert head[5] == 1, (dims, njobs, hooks, p)
    w = np.ctypeslib.as_array(where)[:2 * p["gz"]].reshape(-1, 2).copy()
    return p, [(int(j), int(pc)) for j, pc in w]


def golden_shapes():
    """the 3D scalar shapes of tests/golden/mask_plans.txt with their job counts"""
    out = set()
    for line in open(os.path.join(HERE, "golden", "mask_plans.txt")):
        if line.startswith("#"):
            continue
        nd, scalar, dw, dh, dd, pitch, njobs, reduce = (int(v) for v in line.split("\t")[0].split())
        if nd == 3 and scalar and not reduce:
            out.add(((dw, dh, dd), njobs))
    return sorted(out)


def cases():
    rng = np.random.default_rng(20261017)
    sizes = [2, 6, 8, 16, 40, 64, 70, 72, 100, 128, 130, 256, 258, 264, 512, 520, 1024]
    named = golden_shapes() + [((512, 512, 512), 32), ((256, 256, 256), 16), ((130, 70, 40), 5), ((256, 128, 72), 6)]
    drawn = [(tuple(int(rng.choice(sizes)) if rng.random() < 0.6 else int(rng.integers(1, 513)) * 2 for _ in range(3)), int(rng.integers(1, 41))) for _ in range(300)]
    for dims, njobs in named + drawn:
        for order in (None, 0, 1, 2):
            for sgroup in (None, 1, 2, 3, 4, 7, 100):
                if (dims, njobs) not in named and rng.random() > 1 / 3:      # (every combination on the named shapes, a seeded third on the drawn ones)
                    continue
                hooks = ",".join(k + "=%d" % v for k, v in (("order", order), ("sgroup", sgroup)) if v is not None) or None
                yield dims, njobs, order, sgroup, hooks


def test_every_pair_once_in_every_order(hc):
    seen_orders, marched = set(), 0
    for dims, njobs, order, sgroup, hooks in cases():
        p, where = order_of(hc, dims, njobs, hooks)
        what = (dims, njobs, hooks, p)
        if where is None:
            assert p["sgroup"] == 0, what
            continue
        marched += 1
        npieces, S = p["npieces"], p["sgroup"]
        assert p["gz"] == npieces * njobs and abs(p["njobs"]) == njobs and len(where) == p["gz"], what
        # a bijection onto the (job, piece) pairs
        assert sorted(where) == [(j, pc) for j in range(njobs) for pc in range(npieces)], what
        # which order the hooks ask for
        if order in (0, 1):
            assert S == 0 and (p["njobs"] < 0) == (order == 0), what
        if order == 2:
            assert p["njobs"] < 0 and S >= 1, what
            if sgroup is not None:
                assert S == min(max(sgroup, 1), njobs), what
        if order is None:
            assert (S >= 1) == (p["njobs"] < 0 and njobs > 1), what
            if njobs == 1:
                assert S == 0, what
        if S == 0:
            # today's two orders, literally as the kernel spelled them
            for bz, (job, piece) in enumerate(where):
                if p["njobs"] < 0:
                    want = (bz // npieces, bz % npieces)
                else:
                    pc = bz // njobs
                    want = (bz - pc * njobs, pc)
                assert (job, piece) == want, (what, bz)
            seen_orders.add(0 if p["njobs"] < 0 else 1)
            continue
        # slices in groups, piece by piece inside a group, the slice fastest
        assert 1 <= S <= njobs, what
        seen_orders.add(2)
        if npieces == 1:        # (one piece per column: every order is slice by slice)
            assert where == [(j, 0) for j in range(njobs)], what
            continue
        sizes, pos = [], 0
        while pos < len(where):
            first, piece = where[pos]
            assert piece == 0 and first == sum(sizes), (what, pos)
            size = where.index((first, 1), pos) - pos       # a slice's next piece: exactly one group's slices further on
            assert where[pos:pos + size * npieces] == [(first + s, pc) for pc in range(npieces) for s in range(size)], (what, pos)
            sizes.append(size)
            pos += size * npieces
        assert sum(sizes) == njobs and max(sizes) - min(sizes) <= 1 and max(sizes) <= S and len(sizes) == -(-njobs // S), (what, sizes)
        assert sizes == sorted(sizes, reverse=True), (what, sizes)
    assert seen_orders == {0, 1, 2} and marched > 1000


def test_default_group_sizes(hc):
    # 512^3: 128 workgroups and 2 placement groups per piece of a slice -- four slices are 512 workgroups = one round of 8 placement groups
    p, where = order_of(hc, (512, 512, 512), 32)
    assert (p["njobs"], p["npieces"], p["sgroup"]) == (-32, 23, 4), p
    assert where[:5] == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1)] and where[4 * 23] == (4, 0)
    # 32 slices at a cap of 6: 6, 6, 5, 5, 5, 5
    p, where = order_of(hc, (512, 512, 512), 32, "sgroup=6")
    assert p["sgroup"] == 6 and [j for j, pc in where if pc == 0] == list(range(32))
    assert [where.index((j, 1)) - where.index((j, 0)) for j in range(32)] == [6] * 12 + [5] * 20
    # piece by piece over all slices, and single slices, stay what they were
    for dims, njobs in (((256, 256, 256), 16), ((512, 512, 512), 1), ((256, 256, 256), 1), ((130, 70, 40), 1)):
        p, _ = order_of(hc, dims, njobs)
        assert p["sgroup"] == 0 and (p["njobs"] > 0) == (dims != (512, 512, 512)), (dims, njobs, p)
    p, _ = order_of(hc, (512, 512, 512), 4)         # the slab pass's shape: one group of four
    assert (p["njobs"], p["sgroup"]) == (-4, 4), p
