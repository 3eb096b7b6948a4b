"""A plain `bench.py` run (no --full) sets up, warms up, times the steps, writes --dump-outputs and prints the line -- nothing else.  Its
timed steps are those of a --full run: on the same arguments both dump the same outputs, bit for bit, and the line carries the same
contract keys; the figures that take runs of their own (roofline, per-kernel times, legs, CPU baselines) come with --full only."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config")
FULL_ONLY = ("roofline", "legs", "step_ms", "gpu", "records_d2h", "cpu_all_cores", "value_h2d_inclusive")


def _bench(args, out_dir: Path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", *args, "--dump-outputs", str(out_dir),
                        "--detail-out", str(out_dir / "detail.json")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("workload,args,samples_per_step", [
    ("cfg3", ["--streams", "16", "--track-ms", "200"], 16 * 200 * 8184),
    ("cfg2", ["--streams", "16", "--grid-ms", "16"], 16 * 16 * 2046),
    ("cfg4", ["--grid-ms", "4"], 64 * 4 * 2046),
    ("cfg5", ["--streams", "32"], 10 * 49104),
])
def test_plain_run_times_the_same_steps_as_a_full_one(tmp_path, workload, args, samples_per_step):
    common = ["--workload", workload, *args, "--steps", "2", "--warmup", "1"]
    plain = _bench(common, tmp_path / "plain")
    full = _bench([*common, "--full", "--no-extras", "--no-cpu-baseline", "--no-telemetry"], tmp_path / "full")
    for k in CONTRACT:
        assert k in plain, k
    assert plain["metric"] == full["metric"] and plain["unit"] == "Msamples/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f32" and plain["steps"] == 2 and plain["warmup"] == 1 and plain["config"] == full["config"]
    assert plain["value"] == pytest.approx(samples_per_step / (plain["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert plain["cpu_baseline"] is None and not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert "roofline" in full
    names = sorted(p.name for p in (tmp_path / "plain").glob("*.npy"))
    assert names and names == sorted(p.name for p in (tmp_path / "full").glob("*.npy"))
    for name in names:
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name), err_msg=name)
