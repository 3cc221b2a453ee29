"""bench.py end to end on a small workload: a plain run prints the headline line and nothing beside it (and writes
--dump-outputs); --full adds the legs beside the headline and still prints one line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}
FULL_LEGS = {"roofline", "encoder_stage", "stage_incl_pcie", "stage_incl_files", "coverage_sweep", "cpu_baseline",
             "compression_cost"}


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "200000", *args], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def test_bench_plain_run_prints_the_headline_alone(tmp_path):
    line = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert set(line) == HEADLINE
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0
    assert line["value"] == pytest.approx(200000 * 2 / (line["ms_per_step"] * 2e-3) / 1e6, rel=1e-2)
    # the streams are whole (far below the dump's byte budget): every read once, matched or singleton
    ids = np.concatenate([np.load(tmp_path / "order.npy"), np.load(tmp_path / "order_s.npy")])
    assert np.array_equal(np.sort(ids), np.arange(200000))


def test_bench_full_run_adds_the_legs():
    line = _bench("--steps", "1", "--warmup", "0", "--full", "--cpu-threads", "4", "--cost-sample", "20000",
                  "--choice-sample", "20000", "--sweep-sample", "20000")
    assert HEADLINE | FULL_LEGS <= set(line)
    for k in ("encoder_stage", "stage_incl_pcie", "stage_incl_files", "coverage_sweep"):
        assert "error" not in line[k], (k, line[k])
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["achieved"] > 0
    assert line["cpu_baseline"]["value"] > 0 and "stage_incl_files_error" not in line["cpu_baseline"]
