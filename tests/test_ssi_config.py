"""The scale- and shift-invariant term's config layer without a GPU: loss.ssi_weight / ssi_space /
ssi_trim / ssi_norm are accepted and validated, weight 0 builds no module, --ssi-weight overrides
the file, and loss.si_weight reaches the single-output path only while the term is on."""
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
    from mdemi.train import SSILoss, TrainLoss
    from mdemi.train.builder import LOSS_KEYS, ssi_config
    assert {"ssi_weight", "ssi_space", "ssi_trim", "ssi_norm"} <= set(LOSS_KEYS)
    assert ssi_config({}) == (0.0, "depth", 0.0, "none")
    assert ssi_config(_cfg(ssi_weight=1, ssi_space="disp", ssi_trim=0.2, ssi_norm="gt_var")) == \
        (1.0, "disp", 0.2, "gt_var")
    assert ssi_config(_cfg(ssi_weight=0.5, ssi_trim=0)) == (0.5, "depth", 0.0, "none")
    assert ssi_config(_cfg(ssi_weight=0.5, ssi_trim=0.5))[2] == 0.5
    t = TrainLoss(_cfg(ssi_weight=0.5, ssi_space="disp", ssi_trim=0.25, ssi_norm="gt_var", per_image=True), "adabins")
    assert isinstance(t.ssi, SSILoss) and t.ssi_weight == 0.5
    assert (t.ssi.space, t.ssi.trim, t.ssi.norm, t.ssi.per_image, t.ssi.min_depth) == \
        ("disp", 0.25, "gt_var", True, 0.002)
    assert t.ssi.per_image == t.silog.per_image and t.ssi.min_depth == t.silog.min_depth
    for bad in (-0.5, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match="loss.ssi_weight"):
            TrainLoss(_cfg(ssi_weight=bad), "newcrfs")
    for bad in ("log", "DISP", 1, None, True):
        with pytest.raises(ValueError, match="loss.ssi_space"):
            TrainLoss(_cfg(ssi_weight=0.5, ssi_space=bad), "newcrfs")
        with pytest.raises(ValueError, match="loss.ssi_space"):  # checked even while the term is off
            TrainLoss(_cfg(ssi_space=bad), "newcrfs")
    for bad in (-0.1, 0.51, 1, float("nan"), float("inf"), "0.2", None, True):
        with pytest.raises(ValueError, match="loss.ssi_trim"):
            TrainLoss(_cfg(ssi_weight=0.5, ssi_trim=bad), "newcrfs")
    for bad in ("var", "mad", 0, None, False):
        with pytest.raises(ValueError, match="loss.ssi_norm"):
            TrainLoss(_cfg(ssi_weight=0.5, ssi_norm=bad), "newcrfs")
    with pytest.raises(ValueError, match="space"):
        SSILoss(space="log")
    with pytest.raises(ValueError, match="trim"):
        SSILoss(trim=0.75)
    with pytest.raises(ValueError, match="ssi_wieght"):  # unknown keys are still refused
        TrainLoss(_cfg(ssi_wieght=0.5), "newcrfs")


def test_weight_zero_or_absent_builds_no_module():
    from mdemi.train import TrainLoss, build_from_config
    for off in (_cfg(), _cfg(ssi_weight=0.0), _cfg(ssi_weight=0, ssi_space="disp", ssi_trim=0.2, ssi_norm="gt_var")):
        t = TrainLoss(off, "newcrfs")
        assert t.ssi is None and t.ssi_weight == 0.0
    assert build_from_config(_cfg(), device="meta").criterion.ssi is None
    t = build_from_config(_cfg(ssi_weight=0.25, ssi_trim=0.1), device="meta")
    assert t.criterion.ssi.trim == 0.1 and t.criterion.ssi_weight == 0.25
    with pytest.raises(ValueError, match="loss.ssi_trim"):
        build_from_config(_cfg(ssi_weight=1.0, ssi_trim=0.6), device="meta")


class _Term:
    """Stands in for a loss module: counts its calls and returns a fixed value."""

    def __init__(self, value, per_image=False, min_depth=0.002):
        self.value, self.calls, self.per_image, self.min_depth = value, 0, per_image, min_depth

    def __call__(self, pred, gt):
        self.calls += 1
        return self.value


def _with_terms(cfg, name="newcrfs"):
    import torch
    from mdemi.train import TrainLoss
    t = TrainLoss(cfg, name)
    t.silog = _Term(torch.tensor(3.0))
    if t.ssi is not None:
        t.ssi = _Term(torch.tensor(0.5))
    x = torch.ones(1, 1, 4, 4)
    return t, t(x, x)


def test_si_weight_reaches_the_single_output_path_only_with_the_term_on():
    # off: si_weight is not read, as before
    t, loss = _with_terms(_cfg(si_weight=0.25))
    assert loss.item() == 3.0 and t.silog.calls == 1
    t, loss = _with_terms(_cfg(si_weight=0.0, ssi_weight=0.0))
    assert loss.item() == 3.0 and t.silog.calls == 1
    # on: it weighs SILog; the default 1 leaves it as it is
    t, loss = _with_terms(_cfg(ssi_weight=2.0))
    assert loss.item() == 3.0 + 2.0 * 0.5 and (t.silog.calls, t.ssi.calls) == (1, 1)
    t, loss = _with_terms(_cfg(si_weight=0.25, ssi_weight=2.0))
    assert loss.item() == 0.25 * 3.0 + 2.0 * 0.5 and (t.silog.calls, t.ssi.calls) == (1, 1)
    # si_weight 0: no SILog at all, the loss is the weighted SSI term
    t, loss = _with_terms(_cfg(si_weight=0, ssi_weight=2.0))
    assert loss.item() == 2.0 * 0.5 and (t.silog.calls, t.ssi.calls) == (0, 1)
    # the multi-output model averages both over its outputs and drops SILog in the same way
    import torch
    from mdemi.train import TrainLoss
    outs = [torch.ones(1, 1, 4, 4)] * 3
    for si, want, calls in ((0.7, 0.7 * 3.0 + 2.0 * 0.5, 3), (0, 2.0 * 0.5, 0)):
        t = TrainLoss(_cfg(si_weight=si, ssi_weight=2.0), "oda2_red_order_swin2")
        t.silog, t.ssi = _Term(torch.tensor(3.0)), _Term(torch.tensor(0.5))
        loss = t((outs[0], outs, None), outs[0])
        assert abs(loss.item() - want) < 1e-6 and (t.silog.calls, t.ssi.calls) == (calls, 3)


def test_functional_checks_options_before_anything_runs():
    import torch
    from mdemi import functional as mf
    x = torch.ones(1, 1, 4, 4)  # a CPU tensor: nothing is launched, the checks come first
    with pytest.raises(ValueError, match="space"):
        mf.ssi_loss(x, x, space="log")
    for bad in (-0.1, 0.6, float("nan"), True):
        with pytest.raises(ValueError, match="trim"):
            mf.ssi_loss(x, x, trim=bad)
    with pytest.raises(ValueError, match="norm"):
        mf.ssi_loss(x, x, norm="mad")
    with pytest.raises(ValueError, match="pred and gt"):
        mf.ssi_loss(x, torch.ones(1, 1, 4, 5))


def test_the_binding_declares_the_three_entries():
    from mdemi import _lib
    assert {"mdemi_ssi_workspace_size", "mdemi_ssi_fwd", "mdemi_ssi_bwd"} <= set(_lib.exported_symbols())
    assert (_lib.SSI_DEPTH, _lib.SSI_DISP, _lib.SSI_NORM_NONE, _lib.SSI_NORM_GT_VAR) == (0, 1, 0, 1)
    from mdemi import functional as mf
    assert mf.SSI_SPACES.index("disp") == _lib.SSI_DISP and mf.SSI_NORMS.index("gt_var") == _lib.SSI_NORM_GT_VAR


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


def test_ssi_weight_flag_overrides_the_file(tmp_path):
    from mdemi import run
    from mdemi.train.builder import ssi_config
    assert run._args(["--opt", "x"]).ssi_weight is None
    assert run._args(["--opt", "x", "--ssi-weight", "0.5"]).ssi_weight == 0.5
    opt = run._override(_cfg(ssi_weight=0.25, ssi_space="disp"), run._args(["--opt", "x"]))
    assert ssi_config(opt) == (0.25, "disp", 0.0, "none")
    opt = run._override(_cfg(ssi_weight=0.25, ssi_space="disp"), run._args(["--opt", "x", "--ssi-weight", "0.75"]))
    assert ssi_config(opt) == (0.75, "disp", 0.0, "none")
    opt = run._override(_cfg(ssi_weight=0.25), run._args(["--opt", "x", "--ssi-weight", "0"]))
    assert ssi_config(opt)[0] == 0.0
    opt = run._override({"model": {"name": "newcrfs"}}, run._args(["--opt", "x", "--ssi-weight", "0.5"]))
    assert opt["loss"] == {"ssi_weight": 0.5}
    # a bad value, in the file or on the command line, is refused before anything else is set up
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "", **_cfg(),
           "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="loss.ssi_weight"):
        _run_main(["--opt", str(path), "--ssi-weight", "-1"])
    with pytest.raises(ValueError, match="loss.ssi_weight"):
        _run_main(["--opt", str(path), "--ssi-weight", "nan"])
    cfg["loss"]["ssi_trim"] = 0.7
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="loss.ssi_trim"):
        _run_main(["--opt", str(path), "--ssi-weight", "0.5"])
