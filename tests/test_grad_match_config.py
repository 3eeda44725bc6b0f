"""The gradient-matching term's config layer without a GPU: loss.grad_weight / loss.grad_scales
are accepted and validated, unknown keys and a non-zero sog_weight are still refused, and
--grad-weight overrides the file."""
import json
import os

import pytest

CFG = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
       "dataloader": {"batch_size": 2}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1},
       "loss": {"alpha": 10.0, "beta": 0.15, "per_image": False},
       "eval": {"max_depth_eval": 10, "min_depth_eval": 0.002}}


def _cfg(**loss):
    cfg = json.loads(json.dumps(CFG))
    cfg["loss"].update(loss)
    return cfg


def test_new_keys_are_accepted_and_validated():
    from mdemi.train import GradMatchLoss, TrainLoss
    from mdemi.train.builder import LOSS_KEYS, grad_match_config
    assert {"grad_weight", "grad_scales"} <= set(LOSS_KEYS)
    assert grad_match_config({}) == (0.0, 4)
    assert grad_match_config(_cfg(grad_weight=0.5, grad_scales=2)) == (0.5, 2)
    assert grad_match_config(_cfg(grad_weight=1)) == (1.0, 4)
    for off in (_cfg(), _cfg(grad_weight=0.0), _cfg(grad_weight=0, grad_scales=1)):
        t = TrainLoss(off, "newcrfs")
        assert t.grad is None and t.grad_weight == 0.0
    t = TrainLoss(_cfg(grad_weight=0.5, grad_scales=3, per_image=True), "adabins")
    assert isinstance(t.grad, GradMatchLoss) and t.grad_weight == 0.5
    assert (t.grad.scales, t.grad.per_image, t.grad.min_depth) == (3, True, 0.002)
    assert t.grad.per_image == t.silog.per_image and t.grad.min_depth == t.silog.min_depth
    assert TrainLoss(_cfg(grad_weight=2.0), "newcrfs").grad.scales == 4
    for bad in (-0.5, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match="loss.grad_weight"):
            TrainLoss(_cfg(grad_weight=bad), "newcrfs")
    for bad in (0, 5, -1, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="loss.grad_scales"):
            TrainLoss(_cfg(grad_weight=0.5, grad_scales=bad), "newcrfs")
        with pytest.raises(ValueError, match="loss.grad_scales"):  # checked even while the term is off
            TrainLoss(_cfg(grad_scales=bad), "newcrfs")
    with pytest.raises(ValueError, match="scales"):
        GradMatchLoss(scales=5)


def test_unknown_keys_and_sog_weight_are_still_refused():
    from mdemi.train import TrainLoss
    with pytest.raises(ValueError, match="grad_wieght"):
        TrainLoss(_cfg(grad_wieght=0.5), "newcrfs")
    with pytest.raises(ValueError, match="edge_weight"):
        TrainLoss(_cfg(grad_weight=0.5, edge_weight=1.0), "newcrfs")
    with pytest.raises(ValueError, match="sog_weight"):
        TrainLoss(_cfg(grad_weight=0.5, sog_weight=0.1), "newcrfs")
    assert TrainLoss(_cfg(grad_weight=0.5, sog_weight=0.0, reduction_ratio=4), "newcrfs").grad is not None


def test_build_from_config_on_the_meta_device():
    from mdemi.train import build_from_config
    assert build_from_config(_cfg(), device="meta").criterion.grad is None
    t = build_from_config(_cfg(grad_weight=0.25, grad_scales=2), device="meta")
    assert t.criterion.grad.scales == 2 and t.criterion.grad_weight == 0.25
    with pytest.raises(ValueError, match="loss.grad_weight"):
        build_from_config(_cfg(grad_weight=-1.0), device="meta")


def test_functional_checks_scales_before_anything_runs():
    import torch
    from mdemi import functional as mf
    x = torch.ones(1, 1, 4, 4)  # a CPU tensor: nothing is launched, the check comes first
    for bad in (0, 5, -1, 2.5, True):
        with pytest.raises(ValueError, match="scales"):
            mf.grad_match_loss(x, x, scales=bad)
    with pytest.raises(ValueError, match="pred and gt"):
        mf.grad_match_loss(x, torch.ones(1, 1, 4, 5))


def _run_main(argv):
    from mdemi import run
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    try:
        return run.main(argv)
    finally:  # parse() exports the config's gpu_ids
        if env is None:
            os.environ.pop("HIP_VISIBLE_DEVICES", None)
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = env


def test_grad_weight_flag_overrides_the_file(tmp_path):
    from mdemi import run
    from mdemi.train.builder import grad_match_config
    assert run._args(["--opt", "x"]).grad_weight is None
    assert run._args(["--opt", "x", "--grad-weight", "0.5"]).grad_weight == 0.5
    # absent: the file's value stands; given: it replaces it, 0 switches the term off
    opt = run._override(_cfg(grad_weight=0.25, grad_scales=2), run._args(["--opt", "x"]))
    assert grad_match_config(opt) == (0.25, 2)
    opt = run._override(_cfg(grad_weight=0.25, grad_scales=2), run._args(["--opt", "x", "--grad-weight", "0.75"]))
    assert grad_match_config(opt) == (0.75, 2)
    opt = run._override(_cfg(grad_weight=0.25), run._args(["--opt", "x", "--grad-weight", "0"]))
    assert grad_match_config(opt) == (0.0, 4)
    opt = run._override({"model": {"name": "newcrfs"}}, run._args(["--opt", "x", "--grad-weight", "0.5"]))
    assert opt["loss"] == {"grad_weight": 0.5}
    # a bad value, in the file or on the command line, is refused before anything else is set up
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "", **_cfg(),
           "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="loss.grad_weight"):
        _run_main(["--opt", str(path), "--grad-weight", "-1"])
    with pytest.raises(ValueError, match="loss.grad_weight"):
        _run_main(["--opt", str(path), "--grad-weight", "nan"])
    cfg["loss"]["grad_scales"] = 5
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="loss.grad_scales"):
        _run_main(["--opt", str(path), "--grad-weight", "0.5"])
