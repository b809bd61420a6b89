"""bench.py on a GPU, on a small workload: a plain run prints the headline fields and nothing else, --steps sets the
timed steps, --dump-outputs writes the last timed step's outputs, and a --full run of the same arguments computes the
same step (same inputs, same batch) while adding the figures that moved behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import relmax

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--config", "ref544", "--N", "20000", "--burn-in", "20", "--warmup", "2", "--steps", "5"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
MOVED = ("roofline", "step_roofline", "breakdown_ms_per_step", "reference_run", "reference_logged", "cpu_baseline")


def _bench(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        assert f.endswith(".npy"), f
        a = np.load(os.path.join(d, f))
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        out[f[:-4]] = a
    return out


def test_plain_and_full_runs_dump_the_same_last_step(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    assert all(k in plain for k in HEADLINE) and not any(k in plain for k in MOVED), sorted(plain)
    assert plain["steps"] == 5 and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["ms_per_step"] > 0 and abs(plain["value"] - 2.0 * 200 * 1e3 / plain["ms_per_step"]) <= 1e-9 * plain["value"]

    a = _load(tmp_path / "plain")
    assert set(a) == {"W", "A", "dfavg", "batch_pos_rows", "batch_neg_rows", "batch_pos_dist", "batch_neg_dist",
                      "batch_rho", "batch_kappa"}, sorted(a)
    assert sum(os.path.getsize(tmp_path / "plain" / (k + ".npy")) for k in a) <= 64 << 20
    W = a["W"].astype(np.float64)
    assert W.shape[1] == 544 and a["A"].shape == (544, 544) and a["dfavg"].shape == (544, 544)
    assert relmax(a["A"], W.T @ W) <= 1e-5
    assert a["batch_pos_rows"].shape == (200,) and np.array_equal(a["batch_pos_rows"], np.round(a["batch_pos_rows"]))

    full = _bench(["--full", "--no-cpu-baseline", "--reference-iters", "0", "--dump-outputs", str(tmp_path / "full")])
    assert all(k in full for k in HEADLINE) and "roofline" in full and "breakdown_ms_per_step" in full
    assert full["steps"] == 5 and full["config"]["state_after_run"] is not None
    b = _load(tmp_path / "full")
    assert set(b) == set(a)
    for k in ("batch_pos_rows", "batch_neg_rows"):             # identical inputs: the same rows drawn in the same step
        assert np.array_equal(a[k], b[k]), k
    for k in ("batch_pos_dist", "batch_neg_dist", "A", "dfavg"):   # the HIP events of --full change no arithmetic
        assert relmax(b[k], a[k]) <= 2e-4, (k, relmax(b[k], a[k]))
