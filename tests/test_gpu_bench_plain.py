"""bench.py as a plain run (no --full): the headline's timed passes and nothing else -- one JSON line with the contract
keys, no secondary workloads, CPU baselines, collective record or roofline launches."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_is_the_headline_alone(tmp_path):
    detail = tmp_path / "detail.json"
    env = dict(os.environ, MDG_BENCH_DETAIL=str(detail))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--replicas", "1024"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    out = json.loads(lines[0])
    assert out["metric"] == "MD steps/sec (fwd+adjoint), 108-atom LJ NHC" and out["unit"] == "MD steps/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and abs(out["value"] - 1024 * 49 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    assert not {"secondary", "roofline", "cpu_baseline"} & set(out), sorted(out)
    cfg = out["config"]
    assert cfg["rdf_fused_into_trajectory_kernels"] is True and cfg["replicas_per_gpu"] == 1024
    assert "dist" not in cfg and "phase_ms" not in cfg
    assert not any(k.startswith(("exvol108", "schnet4096", "lj4096", "water192", "single_system")) for k in cfg), sorted(cfg)
    assert not detail.exists(), "the detail file is written by --full runs only"
