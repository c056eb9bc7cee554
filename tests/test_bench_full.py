"""bench.py --full: a plain run reports only what its headline needs; the legs that take runs of their own (the strict record and
config.tolerance, host_boundary, cpu_baseline) come with --full and still honour their --no-* switches."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("strict", "host_boundary", "cpu_baseline")
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "320", "--height", "240", "--views", "3", "--iters", "2",
         "--cpu-width", "64", "--cpu-height", "48"]


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--full", "--no-cpu-baseline"])
    assert a.full is True and a.no_cpu_baseline is True and a.no_host_boundary is False and a.no_strict_record is False


def _run(extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only():
    line = _run([])
    assert all(k in line for k in HEADLINE)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["config"]["mode"] == "fast"
    assert abs(line["value"] - 320 * 240 * 2 / (line["ms_per_step"] * 2e-3) / 1e6) < 1e-6 * line["value"]
    assert not any(k in line for k in FULL_ONLY), sorted(line)
    assert line["config"]["tolerance"] is None


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    line = _run(["--full"])
    assert all(k in line for k in HEADLINE)
    assert all(k in line for k in FULL_ONLY), sorted(line)
    assert line["strict"]["steps"] == 2 and line["strict"]["value"] > 0
    assert 0.5 < line["config"]["tolerance"]["depth_within_1e-2"] <= 1.0
    assert line["host_boundary"]["pinned"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port"
    line = _run(["--full", "--no-strict-record", "--no-host-boundary"])
    assert "strict" not in line and "host_boundary" not in line and "cpu_baseline" in line
    assert line["config"]["tolerance"] is None
