"""Averaged weights (train.ema_decay) through the Trainer, fit and the checkpoint: NeW-CRFs
tiny07 at 64x96, batch 2.  Every comparison between runs is bit equality: the average is
updated by the optimizer's own kernel, so resuming, evaluating in between, capturing the step
or switching the average off must not move a bit of anything else."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _opt(decay=0.9, warmup=True, **train):
    tr = {"grad_norm": 0.1, "epoch": 1, "num_accum": 1, "print_freq": 2, "valid_freq": 4, **train}
    if decay is not None:
        tr.update(ema_decay=decay, ema_warmup=warmup)
    return {"model": {"name": "newcrfs", "version": "tiny07"}, "eval": {"max_depth_eval": 10.0},
            "optimizer": {"lr": 2e-4, "weight_decay": 0.01, "same_lr": True}, "dataloader": {"batch_size": 2},
            "scheduler": {"pct_start": 0.3}, "train": tr}


def _trainer(opt, graph=False, precision=None, steps=10):
    from mdemi.train import build_from_config
    from mdemi.train.telemetry import Telemetry
    torch.manual_seed(0)
    return build_from_config(opt, device=DEV, steps_per_epoch=steps, drop_path=0.0, graph=graph, precision=precision,
                             telemetry=Telemetry(capacity=8))


def _data(n, bad=None):
    g = torch.Generator().manual_seed(3)
    out = [(torch.randn(2, 3, 64, 96, generator=g).to(DEV), (torch.rand(2, 1, 64, 96, generator=g) * 9 + 0.5).to(DEV))
           for _ in range(n)]
    if bad is not None:  # one ground-truth pixel +inf: it passes SILog's gt > min_depth mask
        out[bad][1][1, 0, 17, 23] = float("inf")
    return out


def _state(t, ema=True):
    torch.cuda.synchronize()
    out = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    for i, p in enumerate(t.model.parameters()):
        st = t.optimizer.state.get(p)
        if st is not None:
            out[f"exp_avg.{i}"] = st["exp_avg"].clone()
            out[f"exp_avg_sq.{i}"] = st["exp_avg_sq"].clone()
    if ema and t.ema is not None:
        for k, v in t.ema.module.named_parameters():
            out[f"ema.{k}"] = v.detach().clone()
        out["ema.updates"] = torch.tensor(t.optimizer.ema_updates())
    return out


def _diff(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_build_from_config_makes_the_average_only_when_asked():
    t = _trainer(_opt(decay=None))
    assert t.ema is None and t.optimizer._ema is None
    t = _trainer(_opt())
    assert not t.ema.module.training and not any(p.requires_grad for p in t.ema.module.parameters())
    live = {p.data_ptr() for p in t.model.parameters()} | {b.data_ptr() for b in t.model.buffers()}
    mine = {p.data_ptr() for p in t.ema.module.parameters()} | {b.data_ptr() for b in t.ema.module.buffers()}
    assert not live & mine  # no shared storage
    for (k, p), (k2, e) in zip(t.model.named_parameters(), t.ema.module.named_parameters()):
        assert k == k2 and torch.equal(p, e) and "_mdemi_b16" not in e.__dict__
    assert set(t.optimizer._ema) == {p for p in t.model.parameters() if p.requires_grad}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_resume_is_bit_equal_to_the_straight_run(graph, tmp_path):
    data = _data(8)
    t = _trainer(_opt(), graph=graph)
    for b in data[:4]:
        t.step([b])
    t.epoch = 0
    assert t.optimizer.ema_updates() == 4
    t.save("four", str(tmp_path), 4, 0.5)
    for b in data[4:]:
        t.step([b])
    want = _state(t)
    assert t.optimizer.ema_updates() == 8
    # the file: two more keys, still a weights_only load, still torch.optim.AdamW's layout
    ck = torch.load(tmp_path / "four.pth", map_location="cpu", weights_only=True)
    from mdemi.utils.common_utils import CHECKPOINT_KEYS
    assert set(ck) == set(CHECKPOINT_KEYS) | {"ema_state_dict", "ema_meta"}
    assert ck["ema_meta"] == {"decay": 0.9, "warmup": True, "updates": 4}
    assert list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    assert any(not torch.equal(ck["ema_state_dict"][k], ck["model_state_dict"][k]) for k in ck["model_state_dict"])
    ref = torch.optim.AdamW([torch.nn.Parameter(v.clone()) for v in
                             (p.detach().cpu() for p in t.model.parameters() if p.requires_grad)], lr=1e-3)
    ref.load_state_dict(ck["optimizer_state_dict"])
    # a fresh trainer, resumed
    t2 = _trainer(_opt(), graph=graph)
    addr = [e.data_ptr() for e in t2.ema.module.parameters()]
    t2.resume(str(tmp_path / "four.pth"))
    assert [e.data_ptr() for e in t2.ema.module.parameters()] == addr  # restored in place
    assert t2.optimizer.ema_updates() == 4 and t2.optimizer.step_count == 4
    for b in data[4:]:
        t2.step([b])
    assert _diff(want, _state(t2)) == []


def test_resume_from_a_file_without_an_average_starts_from_the_loaded_weights(tmp_path, capsys):
    data = _data(2)
    t = _trainer(_opt(decay=None))
    t.step([data[0]])
    t.epoch = 0
    t.save("plain", str(tmp_path), 1, 0.5)
    from mdemi.utils.common_utils import CHECKPOINT_KEYS
    assert set(torch.load(tmp_path / "plain.pth", map_location="cpu", weights_only=True)) == set(CHECKPOINT_KEYS)
    t2 = _trainer(_opt())
    t2.step([data[1]])  # the average has moved
    t2.resume(str(tmp_path / "plain.pth"))
    assert "no ema_state_dict" in capsys.readouterr().out
    assert t2.optimizer.ema_updates() == 0
    for (k, p), (_, e) in zip(t2.model.named_parameters(), t2.ema.module.named_parameters()):
        assert torch.equal(p, e), k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_an_evaluation_in_between_changes_nothing(precision):
    from mdemi import functional as mf
    from mdemi.train.builder import build_model
    if precision == "bf16":
        assert mf.get_bf16_storage()
    data = _data(2)

    def evaluate(t):
        t.ema.sync_buffers(t.model)
        with torch.no_grad(), mf.matmul_precision(precision):
            return t.ema.module(data[0][0]).clone()

    a = _trainer(_opt(), precision=precision)
    a.step([data[0]])
    a.step([data[1]])
    b = _trainer(_opt(), precision=precision)
    b.step([data[0]])
    out1 = evaluate(b)
    b.step([data[1]])
    assert _diff(_state(a), _state(b)) == []
    if precision == "bf16":  # the live model's maintained bf16 copies are the cast of its weights
        assert b.optimizer._b16
        for p, c in b.optimizer._b16.items():
            assert torch.equal(c.view(torch.int16), p.detach().to(torch.bfloat16).view(torch.int16))
    # and the second evaluation reads the moved averages, not what the first one cached: it
    # equals a model freshly loaded from the average's state
    out2 = evaluate(b)
    assert not torch.equal(out1, out2)
    fresh = build_model(b.opt, drop_path=0.0).to(DEV).eval()
    fresh.load_state_dict(b.ema.state_dict())
    with torch.no_grad(), mf.matmul_precision(precision):
        want = fresh(data[0][0])
    assert torch.equal(out2, want)


def test_the_live_weights_do_not_know_about_the_average():
    data = _data(3)
    a = _trainer(_opt(decay=0.5, warmup=False))
    b = _trainer(_opt(decay=None))
    for d in data:
        a.step([d])
        b.step([d])
    assert _diff(_state(a, ema=False), _state(b)) == []
    moved = [k for (k, p), (_, e) in zip(a.model.named_parameters(), a.ema.module.named_parameters())
             if not torch.equal(p, e)]
    assert len(moved) > 0.5 * len(list(a.model.parameters()))
    assert a.optimizer.ema_updates() == 3


@pytest.mark.parametrize("which", ["ema", "both"])
def test_fit_validates_the_average(which, tmp_path):
    from mdemi.train.loop import fit
    data = _data(4)
    opt = _opt(ema_validate=which)
    t = _trainer(opt, steps=4)
    seen = []

    def validate(model):
        seen.append("ema" if model is t.ema.module else "model" if model is t.model else "?")
        was = model.training
        model.eval()
        with torch.no_grad():
            d = model(data[0][0])
        model.train(was)
        d = torch.nn.functional.interpolate(d, size=data[0][1].shape[-2:], mode="bilinear")
        return {"abs_rel": ((d - data[0][1]).abs() / data[0][1]).mean().item()}

    code = fit(t, iter([[b] for b in data]), validate, opt, str(tmp_path), steps_per_epoch=4, log=lambda s: None)
    assert code == 0
    assert seen == (["ema"] if which == "ema" else ["ema", "model"])
    assert not t.ema.module.training and t.model.training
    for (k, x), (_, y) in zip(t.model.named_buffers(), t.ema.module.named_buffers()):
        assert torch.equal(x, y), k  # sync_buffers ran
    valid = [r for r in (json.loads(s) for s in open(tmp_path / "log.jsonl")) if r["type"] == "valid"]
    assert [r["weights"] for r in valid] == (["ema"] if which == "ema" else ["ema", "model"])
    assert valid[0]["best"] is True and valid[0]["step"] == 4
    if which == "both":
        assert valid[1]["best"] is False and valid[1]["abs_rel"] != valid[0]["abs_rel"]
    for name in ("latest", "best"):  # chosen on the average's abs_rel, and carrying it
        ck = torch.load(tmp_path / f"{name}.pth", map_location="cpu", weights_only=True)
        assert ck["best"] == valid[0]["abs_rel"] and ck["ema_meta"]["updates"] == 4 and "ema_state_dict" in ck


def test_a_skipped_step_leaves_the_average_where_it_was():
    data = _data(4, bad=2)
    t = _trainer(_opt(nonfinite="skip"))
    assert t.optimizer.skip_nonfinite
    states = []
    for b in data:
        t.step([b])
        states.append(_state(t))
    ema_keys = [k for k in states[0] if k.startswith("ema.")]
    assert [k for k in ema_keys if not torch.equal(states[1][k], states[2][k])] == []
    assert states[2]["ema.updates"].item() == 2 and states[3]["ema.updates"].item() == 3
    for a, b in ((0, 1), (2, 3)):
        moved = [k for k in ema_keys if not torch.equal(states[a][k], states[b][k])]
        assert len(moved) > 0.5 * len(ema_keys), f"step {b + 1}"
    assert t.optimizer.skipped_steps() == (1, 0)
    assert all(torch.isfinite(v).all() for k, v in states[3].items() if v.is_floating_point())
