"""bench.py without --full does only what its headline needs; --full adds the CPU port baseline, the parity checks and the
lines that take runs of their own, and they go on working there."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "parity_full_size", "speedup_vs_cpu_port", "unsorted_input_ms", "unsorted_input_same_rows",
             "reference_default_order", "shard_of_8", "parity_sampled")


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True
    argv = ["--gpus", "2", "--full"]
    assert all(cmd[2:] == argv for cmd, _ in bench.spawn_plan(bench.parse_args(argv), argv, {}))


def _line(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nodes", "20000", "--m", "5", "--steps", "2", "--warmup", "1",
                        *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only():
    out = _line()
    assert all(k in out for k in HEADLINE)
    assert out["metric"] == "eliminated-vertices/sec" and out["unit"] == "vertices/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["steps"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["n_eliminated"] == 10000
    assert not [k for k in FULL_ONLY if k in out]


@pytest.mark.gpu
def test_full_run_checks_parity_and_the_side_lines():
    out = _line("--full", "--cpu-runs", "1")
    assert all(k in out for k in HEADLINE) and out["n_eliminated"] == 10000
    assert out["parity_full_size"] is True
    assert out["cpu_baseline"]["runs"] == 1 and out["cpu_baseline"]["value"] > 0
    assert out["unsorted_input_same_rows"] is True and out["unsorted_input_ms"] > 0
    ro = out["reference_default_order"]
    assert ro["o_v"] == "random" and ro["parity_full_size"] is True and ro["n_eliminated"] == 10000
