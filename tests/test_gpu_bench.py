"""GPU: bench.py end to end at a small size.  A plain run reports the headline only; --full adds the figures that take runs
of their own (the 2 Hz ticks and the CPU baseline are left out here: a minute of idle ticks, a -march=native build)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("host_ingest", "latency", "roofline", "roofline_ragged", "roofline_small_q", "roofline_matrix", "cpu_baseline",
         "stage_us", "hamming_match_GBps")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--records", "2000", *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "relocalization frames/sec @640x480, 10k-landmark DB; Hamming-match HBM GB/s"
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert line["published_in_last_step"] >= 32 and line["frames_in_step"] == 64
    return line


def test_plain_run_reports_the_headline_only(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    for k in MOVED:
        assert line[k] is None, k
    outcome = np.load(tmp_path / "tick_outcome.npy")
    assert outcome.shape == (64,) and (outcome == 0).sum() == line["published_in_last_step"]


def test_full_run_adds_the_other_figures():
    line = _bench("--full", "--no-2hz", "--no-cpu-baseline")
    for k in MOVED:
        if k != "cpu_baseline":
            assert line[k] is not None, k
    assert line["cpu_baseline"] is None
    assert line["roofline"]["in_config"]["scan_launches"] > 0 and line["host_ingest"]["value"] > 0
    assert "tick_global_us" in line["latency"] and "tick_global_2hz_us" not in line["latency"]
