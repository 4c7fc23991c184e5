"""bench.py's plain run: the headline line, the dump, and nothing measured beside them (the rest is --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = ("roofline", "instrumented_block", "frame_latency_ms", "sustained", "extra_configs", "frame_roofline", "traffic_profile", "cpu_baseline")


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_alone(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--blocks", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("Mray/s") and d["unit"] == "Mray/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 4 and d["warmup"] == 2 and d["n_gpus"] == 1 and len(d["blocks_ms_per_step"]) == 2
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["rays_per_frame"] > 1920 * 1080 and d["replay_bit_identical"]
    # value = the counted rays of the timed frames over their time, ms_per_step = that time / --steps
    assert abs(d["value"] - d["rays_per_frame"] / d["ms_per_step"] / 1e3) <= 1e-3 * d["value"]
    assert not [k for k in FULL_ONLY if k in d], [k for k in FULL_ONLY if k in d]
    a = np.load(tmp_path / "tone_mapped.npy")
    assert a.shape == (1080, 1920, 4) and a.dtype == np.float32 and np.isfinite(a).all()
