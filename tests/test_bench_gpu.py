"""bench.py as the command line runs it, on the 64x64 debugging configuration: a plain run carries only the headline figure and
`--dump-outputs` writes the samples of the last timed step."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_plain_bench_run_is_lean_and_dumps_its_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--tiny", "--batch", "2",
                        "--timesteps", "4", "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["dtype"] == "bf16"
    assert line["unit"] == "images/sec" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    assert not {"roofline", "cpu_baseline", "parity"} & set(line)            # those legs run under --full only
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["samples.npy"]
    x = np.load(tmp_path / "out" / "samples.npy")
    assert x.dtype == np.float32 and x.shape == (2, 3, 64, 64)
    assert np.isfinite(x).all() and np.abs(x).max() <= 1.0 and x.std() > 0    # dynamic clip: finished samples lie in [-1, 1]
