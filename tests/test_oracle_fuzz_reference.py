"""The oracle against THE REFERENCE ITSELF on seeded random series (not gpu): oracle/_ref/ftk_ref_driver -- hguo/ftk's own trackers
compiled from its headers by oracle/Makefile -- tracked each series in `file` mode; the C restatement must give the same records
(bit for bit), factors included.  Pins the oracle beyond the committed fixtures.  What the reference returned is recorded in
tests/golden/fuzz_reference.json (tests/golden/make_golden_fuzz.py: record counts, factors, digests of the records)."""
import json
import os

import numpy as np
import pytest

from common import GOLDEN, records_digest
from test_gpu_fuzz import _field, _vector_series, KINDS

SEEDS = range(12)


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "fuzz_reference.json")) as f:
        return json.load(f)["seeds"]


def fuzz_cases(seed):
    """the four random series of a seed -> (steps, nd, nv, the reference driver's environment, the oracle's options, what)"""
    rng = np.random.default_rng(7000 + seed)
    for case in range(4):
        nd = int(rng.choice([2, 3]))
        nv = int(rng.choice([1, nd]))
        nt = int(rng.integers(2, 7))
        if nd == 2:
            dims = (int(rng.choice([16, 24, 40, 64, 130])) + int(rng.integers(0, 2)), int(rng.integers(9, 60)))
        else:
            dims = (int(rng.choice([8, 16, 24, 40])) + int(rng.integers(0, 2)), int(rng.integers(7, 30)), int(rng.integers(7, 18)))
        sp = tuple(reversed(dims))
        kind = str(rng.choice(KINDS))
        steps = _field(rng, (nt,) + sp, kind) if nv == 1 else _vector_series(rng, nt, sp, kind)
        robust = bool(rng.random() < 0.85) or nd == 2
        type_filter = int(rng.choice([1, 2, 4, 8, 16, 6, 24])) if (nd == 2 and rng.random() < 0.25) else None
        degrees = bool(nd == 2 and rng.random() < 0.15)
        env = {}
        if not robust:
            env["FTK_REF_NO_ROBUST"] = "1"
        if type_filter is not None:
            env["FTK_REF_TYPE_FILTER"] = str(type_filter)
        if degrees:
            env["FTK_REF_DEGREES"] = "1"
        what = f"seed {seed} case {case}: nd {nd} nv {nv} dims {dims} nt {nt} {kind} robust {robust} filter {type_filter} degrees {degrees}"
        yield steps, nd, nv, env, dict(robust=robust, type_filter=type_filter, compute_degrees=degrees), what


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_equals_the_real_reference_on_random_series(oracle, recorded, seed):
    want = recorded[str(seed)]
    cases = list(fuzz_cases(seed))
    assert len(cases) == len(want)
    for (steps, nd, nv, _env, opts, what), ref in zip(cases, want):
        got, gf, _ = oracle.track(steps, nd, nv, **opts, tag_mode=oracle.TAG_REFERENCE, nthreads=8)
        assert [int(f) for f in gf] == ref["factors"], what + f": factors {gf} vs {ref['factors']}"
        assert len(got) == ref["records"], what + f": {len(got)} records, the reference returned {ref['records']}"
        assert records_digest(got) == ref["records_sha256"], what + ": the records are not bit-identical to the reference's"
