"""Averaged weights (train.ema_decay) without a GPU: the config keys, build_from_config on the
meta device, the checkpoint's two extra keys and the command lines."""
import json
import os

import pytest
import torch

CFG = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
       "dataloader": {"batch_size": 2}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1},
       "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001}}


def _cfg(**train):
    cfg = json.loads(json.dumps(CFG))
    cfg["train"].update(train)
    return cfg


def test_key_validation():
    from mdemi.train.ema import ema_config
    assert ema_config({}) == (None, False, "ema")
    assert ema_config({"train": {"ema_decay": None}}) == (None, False, "ema")
    assert ema_config(_cfg(ema_decay=0.999, ema_warmup=True, ema_validate="both")) == (0.999, True, "both")
    assert ema_config(_cfg(ema_decay=0)) == (0.0, False, "ema")
    for bad in (1.0, -0.1, "0.9", True, 2, float("nan")):
        with pytest.raises(ValueError, match="train.ema_decay"):
            ema_config(_cfg(ema_decay=bad))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="train.ema_warmup"):
            ema_config(_cfg(ema_decay=0.9, ema_warmup=bad))
    for bad in ("model", "EMA", None, True):
        with pytest.raises(ValueError, match="train.ema_validate"):
            ema_config(_cfg(ema_decay=0.9, ema_validate=bad))


def test_build_from_config_on_the_meta_device():
    from mdemi.train import ModelEma, build_from_config
    t = build_from_config(_cfg(), device="meta")
    assert t.ema is None and t.optimizer._ema is None
    t = build_from_config(_cfg(ema_decay=None), device="meta")
    assert t.ema is None
    t = build_from_config(_cfg(ema_decay=0.99, ema_warmup=True), device="meta")
    assert isinstance(t.ema, ModelEma) and (t.ema.decay, t.ema.warmup) == (0.99, True)
    assert not t.ema.module.training and not any(p.requires_grad for p in t.ema.module.parameters())
    assert (t.optimizer._ema_decay, t.optimizer._ema_warmup) == (0.99, True)
    live = dict(t.model.named_parameters())
    mine = dict(t.ema.module.named_parameters())
    assert list(live) == list(mine)
    assert {id(p) for p in t.optimizer._ema} == {id(p) for p in live.values() if p.requires_grad}
    for k, p in live.items():
        assert t.optimizer._ema[p] is mine[k] and mine[k].shape == p.shape
    assert t.optimizer.ema_updates() == 0
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.5), dict(ema_decay="0.9"),
                dict(ema_decay=0.9, ema_validate="raw")):
        with pytest.raises(ValueError, match="train.ema_"):
            build_from_config(_cfg(**bad), device="meta")


def test_set_ema_bumps_the_layout_and_checks_its_arguments():
    from mdemi.train import FusedAdamW
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    opt = FusedAdamW(ps, lr=1e-3)
    with pytest.raises(RuntimeError, match="set_ema"):
        opt.ema_updates()
    v = opt.layout_version
    opt.set_ema({ps[0]: torch.zeros(3)}, 0.9, warmup=True)
    assert opt.layout_version == v + 1 and opt.ema_updates() == 0
    opt.set_ema_updates(7)
    assert opt.ema_updates() == 7
    for decay in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            opt.set_ema({ps[0]: torch.zeros(3)}, decay)
    with pytest.raises(ValueError, match="shape"):
        opt.set_ema({ps[1]: torch.zeros(4)}, 0.9)
    with pytest.raises(ValueError, match="fp32"):
        opt.set_ema({ps[0]: torch.zeros(3, dtype=torch.float64)}, 0.9)
    with pytest.raises(ValueError, match="not a parameter"):
        opt.set_ema({torch.nn.Parameter(torch.zeros(3)): torch.zeros(3)}, 0.9)


def test_checkpoint_round_trip_of_the_two_keys(tmp_path):
    from mdemi.utils.common_utils import CHECKPOINT_KEYS, load_checkpoint, save_checkpoint

    class Opt:
        def state_dict(self):
            return {"state": {}, "param_groups": []}

    torch.manual_seed(0)
    model, avg = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    extra = {"ema_state_dict": avg.state_dict(), "ema_meta": {"decay": 0.999, "warmup": True, "updates": 12}}
    save_checkpoint("with", model, Opt(), 1, 5, 0.25, str(tmp_path), extra=extra)
    save_checkpoint("without", model, Opt(), 1, 5, 0.25, str(tmp_path))
    ck = torch.load(tmp_path / "with.pth", map_location="cpu", weights_only=True)
    assert list(ck) == list(CHECKPOINT_KEYS) + ["ema_state_dict", "ema_meta"]
    assert ck["ema_meta"] == extra["ema_meta"]
    assert all(torch.equal(ck["ema_state_dict"][k], v) for k, v in avg.state_dict().items())
    assert all(torch.equal(ck["model_state_dict"][k], v) for k, v in model.state_dict().items())
    assert list(torch.load(tmp_path / "without.pth", weights_only=True)) == list(CHECKPOINT_KEYS)
    # a loader that does not know the keys ignores them
    m2 = torch.nn.Linear(3, 2)
    got = load_checkpoint(str(tmp_path / "with.pth"), m2)
    assert torch.equal(m2.weight, model.weight) and got["ema_meta"]["updates"] == 12
    with pytest.raises(ValueError, match="shadow"):
        save_checkpoint("bad", model, Opt(), 1, 5, 0.25, str(tmp_path), extra={"best": 1.0})
    with pytest.raises(TypeError):  # keyword-only
        save_checkpoint("bad", model, Opt(), 1, 5, 0.25, str(tmp_path), None, None, False, extra)


def test_trainer_save_and_resume_carry_the_average(tmp_path):
    """Trainer.save / resume on CPU tensors with a stand-in optimizer: the average and its
    update count come back in place."""
    from mdemi.train import ModelEma
    from mdemi.train.builder import Trainer

    class Opt:
        capturable, step_count, updates = False, 0, 3

        def state_dict(self):
            return {"state": {}, "param_groups": []}

        def load_state_dict(self, sd):
            pass

        def ema_updates(self):
            return self.updates

        def set_ema_updates(self, n):
            self.updates = n

    def make():
        torch.manual_seed(1)
        model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
        ema = ModelEma.__new__(ModelEma)
        ema.decay, ema.warmup = 0.9, False
        ema.module = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2)).eval().requires_grad_(False)
        ema.module.load_state_dict(model.state_dict())
        return Trainer({"train": {}}, model, None, Opt(), None, ema=ema)

    t = make()
    with torch.no_grad():
        t.ema.module[0].weight.add_(1.0)
        t.model[1].running_mean.add_(0.5)
    t.ema.sync_buffers(t.model)
    assert torch.equal(t.ema.module[1].running_mean, t.model[1].running_mean)
    assert set(t.ema.pairs(t.model).values()) == set(t.ema.module.parameters())
    t.save("ck", str(tmp_path), 2, 0.5)
    ck = torch.load(tmp_path / "ck.pth", weights_only=True)
    assert ck["ema_meta"] == {"decay": 0.9, "warmup": False, "updates": 3}
    t2 = make()
    t2.optimizer.updates = 0
    w = t2.ema.module[0].weight
    t2.resume(str(tmp_path / "ck.pth"))
    assert t2.ema.module[0].weight is w and torch.equal(w, t.ema.module[0].weight)
    assert not torch.equal(w, t2.model[0].weight) and t2.optimizer.updates == 3


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


def test_command_lines(tmp_path):
    from mdemi import predict, run
    from mdemi.utils.common_utils import save_checkpoint
    assert run._args(["--opt", "x"]).ema_decay is None and run._args(["--opt", "x"]).ema is False
    assert run._args(["--opt", "x", "--ema-decay", "0.999"]).ema_decay == 0.999
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "",
           "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}, **{k: v for k, v in _cfg().items() if k != "dataset"}}
    cfg["dataloader"]["num_workers"] = 0
    path = tmp_path / "cfg.json"
    # a bad key, in the file or on the command line, is refused before anything else is set up
    path.write_text(json.dumps({**cfg, "train": {"epoch": 1, "ema_decay": 1.0}}))
    with pytest.raises(ValueError, match="train.ema_decay"):
        _run_main(["--opt", str(path)])
    path.write_text(json.dumps({**cfg, "train": {"epoch": 1, "ema_decay": 0.9, "ema_validate": "best"}}))
    with pytest.raises(ValueError, match="train.ema_validate"):
        _run_main(["--opt", str(path)])
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="train.ema_decay"):
        _run_main(["--opt", str(path), "--ema-decay", "1.5"])
    # --test --ema on a file without an average
    model = torch.nn.Linear(3, 2)
    save_checkpoint("plain", model, None, 0, 1, 0.5, str(tmp_path), model_only=True)
    with pytest.raises(SystemExit) as e:
        _run_main(["--opt", str(path), "--test", "--ema", "--checkpoint", str(tmp_path / "plain.pth")])
    assert "ema_state_dict" in str(e.value) and "plain.pth" in str(e.value)
    with pytest.raises(SystemExit, match="--test"):
        _run_main(["--opt", str(path), "--ema"])
    # mdemi.predict's loader: the same message, and the average when it is there
    with pytest.raises(SystemExit, match="ema_state_dict"):
        predict._load_weights(torch.nn.Linear(3, 2), str(tmp_path / "plain.pth"), ema=True)
    avg = torch.nn.Linear(3, 2)
    save_checkpoint("avg", model, None, 0, 1, 0.5, str(tmp_path), model_only=True,
                    extra={"ema_state_dict": avg.state_dict(), "ema_meta": {"decay": 0.9, "warmup": False, "updates": 1}})
    m = torch.nn.Linear(3, 2)
    predict._load_weights(m, str(tmp_path / "avg.pth"), ema=True)
    assert torch.equal(m.weight, avg.weight)
    predict._load_weights(m, str(tmp_path / "avg.pth"))
    assert torch.equal(m.weight, model.weight)
