"""bench.py's plain run and --dump-outputs on the GPU, at a tiny workload (NeW-CRFs tiny07,
64x96, batch 2, given as a --config file): the plain line carries the headline figure and
ms_per_step and none of the --full measurements, --steps sets the timed steps, and the dumped
arrays are float32, finite, within the size limit and hold the loss the line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = {"model": {"name": "newcrfs", "version": "tiny07"},
        "loss": {"alpha": 10.0, "beta": 0.15, "per_image": False},
        "dataset": {"data_type": "NYU"}, "dataloader": {"batch_size": 2},
        "optimizer": {"lr": 2e-5, "weight_decay": 0.0},
        "scheduler": {"name": "onecycle", "pct_start": 0.3, "div_factor": 25, "final_div_factor": 100},
        "train": {"epoch": 1, "num_accum": 1, "grad_norm": 0.1},
        "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001}}


def test_plain_run_dumps_last_step_outputs(tmp_path):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY))
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", str(cfg), "--height", "64", "--width", "96", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "images/sec" and rec["higher_is_better"]
    assert rec["dtype"] == "fp32" and rec["ms_per_step"] > 0
    # value is images per second of the timed steps: batch 2 per ms_per_step (both rounded in the line)
    assert rec["value"] == pytest.approx(2 / (rec["ms_per_step"] * 1e-3), rel=0.02)
    # a plain run measures nothing beyond the headline
    assert rec["roofline"] is None and rec["cpu_baseline"] is None
    assert "secondary" not in rec and "secondaries" not in rec and "gemm_all" not in rec
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(arrays) == ["exp_avg", "exp_avg_sq", "loss", "params"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    assert arrays["loss"].shape == (1,) and float(arrays["loss"][0]) == pytest.approx(rec["loss"], abs=1e-5)
    n = arrays["params"].size
    assert n > 1000 and arrays["exp_avg"].size == n and arrays["exp_avg_sq"].size == n
    # the sampled state is the trained one: gradients reached the moments
    assert np.count_nonzero(arrays["exp_avg"]) > n // 2 and (arrays["exp_avg_sq"] >= 0).all()
