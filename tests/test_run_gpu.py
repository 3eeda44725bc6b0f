"""python -m mdemi.run end to end on the GPU: train 2 epochs of 8 NYU-format frames with the
tiny07 NeW-CRFs at 64x96, validate, checkpoint, test and resume."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

METRICS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")


def _write_frames(root, n, seed, prefix):
    """NYU-format frames: an RGB JPEG and a 16-bit PNG depth in millimetres (480x640)."""
    from PIL import Image
    H, W = 480, 640
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    names = []
    for i in range(n):
        ph = rng.uniform(0, 6.28, 3)
        rgb = np.stack([127 + 80 * np.sin(xx / (37 + 11 * c) + yy / (53 - 7 * c) + ph[c]) for c in range(3)], -1)
        rgb = np.clip(rgb + rng.normal(0, 12, rgb.shape), 0, 255).astype(np.uint8)
        dep = (1000 * (0.5 + 9.0 * (xx / W) * (0.6 + 0.4 * np.sin(yy / 41 + ph[0])) ** 2)).astype(np.uint16)
        Image.fromarray(rgb).save(os.path.join(root, f"{prefix}_rgb_{i:04d}.jpg"), quality=95)
        Image.fromarray(dep).save(os.path.join(root, f"{prefix}_depth_{i:04d}.png"))
        names.append(f"/{prefix}_rgb_{i:04d}.jpg /{prefix}_depth_{i:04d}.png 518.8579\n")
    return names


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("run")
    data = root / "data"
    lists = root / "lists" / "NYU"
    data.mkdir()
    lists.mkdir(parents=True)
    (lists / "nyu_train_36k.txt").write_text("".join(_write_frames(str(data), 8, 0, "train")))
    (lists / "nyu_test.txt").write_text("".join(_write_frames(str(data), 2, 1, "test")))
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    yield root
    if env is None:  # common_utils.parse exports the config's gpu_ids
        os.environ.pop("HIP_VISIBLE_DEVICES", None)
    else:
        os.environ["HIP_VISIBLE_DEVICES"] = env


def _config(root, name):
    cfg = {"gpu_ids": [0], "output_dir": str(root / name), "checkpoint": "",
           "model": {"name": "newcrfs", "version": "tiny07"},
           "loss": {"alpha": 10.0, "beta": 0.15, "per_image": False},
           "dataset": {"data_type": "NYU", "data_path": str(root / "data"), "use_right": False, "img_size": [64, 96]},
           "dataloader": {"batch_size": 2, "num_workers": 0},
           "optimizer": {"lr": 2e-4, "weight_decay": 0.01},
           "scheduler": {"name": "onecycle", "pct_start": 0.3, "div_factor": 25, "final_div_factor": 100},
           "train": {"print_freq": 1, "valid_freq": 4, "epoch": 2, "num_accum": 1, "grad_norm": 0.1},
           "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001, "garg_crop": False, "eigen_crop": True,
                    "flip_eval": False}}
    path = root / f"{name}.json"
    path.write_text(json.dumps(cfg))
    return path


def _run(root, name, *extra):
    from mdemi import run
    code = run.main(["--opt", str(_config(root, name)), "--list-root", str(root / "lists"), "--drop-path", "0",
                     *extra])
    log = [json.loads(s) for s in open(root / name / "log.jsonl")]
    return code, log


@pytest.fixture(scope="module")
def run_a(workdir):
    return _run(workdir, "a")


def test_train_logs_validates_and_checkpoints(workdir, run_a):
    from mdemi.utils.common_utils import CHECKPOINT_KEYS
    code, log = run_a
    assert code == 0
    train = [r for r in log if r["type"] == "train"]
    valid = [r for r in log if r["type"] == "valid"]
    assert [r["step"] for r in train] == list(range(1, 9))
    assert [(r["epoch"], r["iter"]) for r in train] == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 1), (1, 2), (1, 3), (1, 4)]
    for r in train:
        for k in ("loss", "grad_norm", "grad_norm_max", "param_norm", "lr", "images_per_sec"):
            assert math.isfinite(r[k]) and r[k] > 0, (k, r)
        assert r["dropped"] == 0
    assert [r["step"] for r in valid] == [4, 8]
    for r in valid:
        assert set(METRICS) <= set(r) and all(math.isfinite(r[k]) for k in METRICS)
    assert valid[0]["best"] is True
    out = workdir / "a"
    latest = torch.load(out / "latest.pth", map_location="cpu", weights_only=True)
    best = torch.load(out / "best.pth", map_location="cpu", weights_only=True)
    assert set(latest) == set(best) == set(CHECKPOINT_KEYS)
    assert (latest["epoch"], latest["iter"]) == (1, 4)
    b = [r for r in valid if r["best"]][-1]
    assert (best["epoch"], best["iter"]) == (b["epoch"], b["iter"]) == (best["best_epoch"], best["best_iter"])
    assert best["best"] == latest["best"] == b["abs_rel"] == min(r["abs_rel"] for r in valid)
    assert latest["optimizer_state_dict"] is not None
    assert json.load(open(out / "option.json"))["train"]["valid_freq"] == 4


def test_test_mode_reproduces_the_logged_metrics(workdir, run_a):
    _, log = run_a
    want = [r for r in log if r["type"] == "valid" and r["best"]][-1]
    code, tlog = _run(workdir, "t", "--test", "--checkpoint", str(workdir / "a" / "best.pth"))
    assert code == 0
    got = tlog[-1]
    assert got["type"] == "test"
    for k in METRICS:
        assert got[k] == want[k], k  # fixed-order metric sums, bit-identical GEMM variants


def test_resume_continues_the_identical_run(workdir, run_a):
    code, log_b = _run(workdir, "b", "--max-steps", "4")
    assert code == 0 and [r["step"] for r in log_b if r["type"] == "train"] == [1, 2, 3, 4]
    code, log_c = _run(workdir, "c", "--checkpoint", str(workdir / "b" / "latest.pth"))
    assert code == 0 and [r["step"] for r in log_c if r["type"] == "train"] == [5, 6, 7, 8]
    a = torch.load(workdir / "a" / "latest.pth", map_location="cpu", weights_only=True)
    c = torch.load(workdir / "c" / "latest.pth", map_location="cpu", weights_only=True)
    assert (c["epoch"], c["iter"]) == (a["epoch"], a["iter"])
    for k, va in a["model_state_dict"].items():
        assert torch.equal(va, c["model_state_dict"][k]), k
    _, log_a = run_a
    for ra, rc in zip([r for r in log_a if r["type"] == "train"][4:], [r for r in log_c if r["type"] == "train"]):
        assert ra["loss"] == rc["loss"] and ra["grad_norm"] == rc["grad_norm"]
