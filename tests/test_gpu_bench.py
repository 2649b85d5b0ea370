"""bench.py's two modes on a 32^3 grid: a plain run stops after its timed steps, --full adds the other legs to the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def bench_line(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "32", "--steps", "6",
                        "--warmup", "2", "--dump-outputs", str(out), *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_plain_run_stops_after_the_timed_steps_and_full_adds_the_rest(tmp_path):
    plain, plain_dir = bench_line(tmp_path, "plain")
    full, full_dir = bench_line(tmp_path, "full", "--full")
    for line in (plain, full):
        assert all(k in line for k in HEADLINE)
        assert line["unit"] == "time-steps/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
        assert line["value"] > 0 and line["steps"] == 6 and line["warmup"] == 2
        assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1.0  # both rounded: 2 and 4 decimals
        assert line["dumped_outputs"]["time_index"] == 8
    assert plain["metric"] == full["metric"]
    # nothing that takes a run of its own in the plain line
    assert "cpu_baseline" not in plain and "c4_512" not in plain["config"]
    assert plain["roofline"]["kernel"] == "step"
    assert not {"kernels", "entry_points", "measured_copy_gbs"} & set(plain["roofline"])
    # all of it behind --full
    assert full["cpu_baseline"]["value"] > 0
    assert full["roofline"]["measured_copy_gbs"] > 0
    assert full["roofline"]["kernels"] and full["roofline"]["entry_points"]
    assert full["roofline"]["step"]["alg_bytes"] == plain["roofline"]["alg_bytes"]
    # the timed steps are the same steps: what they leave behind does not depend on the mode
    assert plain["dumped_outputs"]["files"] == full["dumped_outputs"]["files"]
    for f in plain["dumped_outputs"]["files"]:
        a, b = np.load(plain_dir / f), np.load(full_dir / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
