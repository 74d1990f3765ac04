"""bench.py without --full: set-up, warm-up, exactly --steps timed passes and the line -- and `--dump-outputs DIR`, the records and
factors of the last timed pass as float64 .npy files, which must be the records the full run hands to pass 2 (`--dump-merged`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "small3", "--warmup", "1", *extra], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "ONE JSON line"
    return json.loads(lines[0])


def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path):
    plain = _bench("--steps", "5", "--dump-outputs", str(tmp_path / "out"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 5 and len(plain["ms_per_step_samples"]) == 5 and plain["ms_per_step"] > 0 and plain["value"] > 0
    for k in ("configs", "cpu_baseline", "streaming_tracker", "patched_reference_tracker"):     # (what --full adds)
        assert k not in plain, k
    assert plain["sustained"] is None and plain["pass2"] is None and plain["single_pass_latency_ms"] is None

    full = _bench("--steps", "2", "--full", "--no-cpu-baseline", "--no-other-configs", "--no-streaming-tracker", "--dump-merged", str(tmp_path / "full.npz"))
    assert full["check"]["ok"] and full["pass2"] is not None, full["check"]
    ref = np.load(tmp_path / "full.npz")["records"]

    def get(name):
        a = np.load(tmp_path / "out" / (name + ".npy"))
        assert a.dtype == np.float64
        return a
    assert int(get("n_records")[0]) == len(ref) == plain["check"]["hits"] > 0
    assert np.array_equal(get("records_row"), np.arange(len(ref)))
    tag = (get("records_tag_hi").astype(np.uint64) << np.uint64(32)) | get("records_tag_lo").astype(np.uint64)
    assert np.array_equal(tag, ref["tag"])
    for f in ("x", "t", "scalar"):
        assert np.array_equal(get("records_" + f), ref[f]), f
    for f in ("type", "aux"):
        assert np.array_equal(get("records_" + f).astype(np.uint32), ref[f]), f
    factors = (get("factors_hi").astype(np.uint64) << np.uint64(32)) | get("factors_lo").astype(np.uint64)
    assert len(factors) == 8 and int(np.log2(factors.max())) == full["config"]["nbits"]      # (small3: 8 timesteps)
