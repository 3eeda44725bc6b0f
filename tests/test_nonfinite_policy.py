"""train.nonfinite "skip" without a GPU: fit()'s handling of skipped steps (fakes in the style
of test_run_loop.py), config / CLI validation, Telemetry.drain(raise_on_nonfinite=False) on a
hand-made ring, and the optimizer state's "schedule_step"."""
import json
import math
import os

import numpy as np
import pytest
import torch

from mdemi import _lib as L
from mdemi.train.loop import fit
from mdemi.train.telemetry import Drained, NonFiniteStep, StepRecord, Telemetry

GRAD, LOSS = L.STEP_GRAD_NONFINITE, L.STEP_LOSS_NONFINITE


class FakeTelemetry:
    """flags: {record index: flags}.  A GRAD-flagged record carries the non-finite values the
    device would have recorded, so a mean that included it would not be finite."""

    def __init__(self, flags):
        self.records, self.seen, self.flags = [], 0, dict(flags)

    def push(self, loss):
        i = len(self.records)
        f = self.flags.get(i, 0)
        if f & GRAD:
            rec = StepRecord(float("nan"), float("inf"), i, f)
        elif f & LOSS:
            rec = StepRecord(float("inf"), 4.0, i, f)
        else:
            rec = StepRecord(loss, 4.0, i, 0)
        self.records.append(rec)

    def drain(self, raise_on_nonfinite=True):
        new = self.records[self.seen:]
        if raise_on_nonfinite and any(r.flags for r in self.records):
            raise NonFiniteStep(min(r.index for r in self.records if r.flags))
        self.seen = len(self.records)
        return Drained(new, 0, self.seen)


class FakeOptimizer:
    """Keeps mdemi_guard_state's (skipped, consecutive) as the device would."""

    def __init__(self, norm=3.0):
        self.norm, self.skipped, self.consecutive = norm, 0, 0

    def param_norm(self):
        return torch.tensor(self.norm)

    def skipped_steps(self):
        return self.skipped, self.consecutive


class FakeScheduler:
    def get_last_lr(self):
        return [1e-5, 1e-4]


class FakeTrainer:
    def __init__(self, telemetry, norm=3.0, buffers_ok=True):
        self.telemetry, self.optimizer, self.scheduler = telemetry, FakeOptimizer(norm), FakeScheduler()
        self.epoch, self.steps, self.saves, self.buffers_ok = 0, 0, [], buffers_ok

    def step(self, batches):
        f = self.telemetry.flags.get(self.steps, 0)
        self.steps += 1
        if f & GRAD:
            self.optimizer.skipped += 1
            self.optimizer.consecutive += 1
        else:
            self.optimizer.consecutive = 0
        self.telemetry.push(float(self.steps))

    def buffers_finite(self):
        return self.buffers_ok

    def save(self, prefix, save_dir, current_iter, best_value, best_epoch=None, best_iter=None, model_only=False):
        self.saves.append((prefix, self.steps))
        with open(os.path.join(save_dir, prefix + ".pth"), "w") as f:
            f.write(str(self.steps))


def _opt(**train):
    return {"dataloader": {"batch_size": 2},
            "train": {"print_freq": 2, "valid_freq": 3, "epoch": 2, "num_accum": 1, **train}}


def _fit(tmp_path, flags, opt, **trainer_kw):
    tel = FakeTelemetry(flags)
    tr = FakeTrainer(tel, **trainer_kw)
    lines = []
    code = fit(tr, iter([[("img", "gt")]] * 100), lambda: {"abs_rel": 0.5, "rmse": 1.0}, opt, str(tmp_path),
               steps_per_epoch=5, log=lines.append)
    log = [json.loads(s) for s in open(tmp_path / "log.jsonl")] if (tmp_path / "log.jsonl").exists() else []
    return code, tr, log, lines


def test_fit_skip_mode_continues_counts_and_keeps_skipped_steps_out_of_the_means(tmp_path):
    # records 2 and 6 (global steps 3 and 7) were skipped; record 4 (step 5) has a non-finite
    # loss only: it was applied
    code, tr, log, lines = _fit(tmp_path, {2: GRAD | LOSS, 4: LOSS, 6: GRAD}, _opt(nonfinite="skip"))
    assert code == 0 and tr.steps == 10
    train = [r for r in log if r["type"] == "train"]
    assert [r["step"] for r in train] == [2, 4, 6, 8, 10]
    assert [r["skipped"] for r in train] == [0, 1, 0, 1, 0]
    assert [r["skipped_total"] for r in train] == [0, 1, 1, 2, 2]
    # window means over the applied steps with a finite loss: (1,2) (4) (6) (8) (9,10)
    assert [r["loss"] for r in train] == [1.5, 4.0, 6.0, 8.0, 9.5]
    assert all(r["grad_norm"] == r["grad_norm_max"] == 2.0 for r in train)
    assert set(train[0]) == {"type", "epoch", "iter", "step", "loss", "grad_norm", "grad_norm_max", "param_norm", "lr",
                             "images_per_sec", "dropped", "skipped", "skipped_total"}
    assert [r for r in log if r["type"] == "skipped"] == [{"type": "skipped", "step": 3, "epoch": 0, "iter": 3},
                                                          {"type": "skipped", "step": 7, "epoch": 1, "iter": 2}]
    assert [r for r in log if r["type"] == "nonfinite_loss"] == [{"type": "nonfinite_loss", "step": 5, "epoch": 0,
                                                                  "iter": 5}]
    # validation and checkpoints go on as usual
    assert [r["step"] for r in log if r["type"] == "valid"] == [3, 6, 9, 10]
    assert [s for p, s in tr.saves if p == "latest"] == [3, 6, 9, 10]
    assert len(lines) == len(log)


def test_fit_default_policy_has_no_skip_fields_and_still_stops(tmp_path):
    code, tr, log, _ = _fit(tmp_path / "a", {}, _opt())
    assert code == 0
    assert all("skipped" not in r and "skipped_total" not in r for r in log if r["type"] == "train")
    code, tr, log, lines = _fit(tmp_path / "b", {4: GRAD}, _opt())
    assert code == 1 and tr.steps == 6
    assert tr.saves == [("latest", 3), ("best", 3)]
    assert log[-1] == {"type": "nonfinite", "step": 5, "epoch": 0, "iter": 5, "count": 1}


def test_fit_skip_mode_stops_once_the_streak_exceeds_the_limit(tmp_path):
    # steps 4..7 skipped; with a limit of 2 the drain at step 6 sees a streak of 3
    flags = {i: GRAD for i in (3, 4, 5, 6)}
    code, tr, log, lines = _fit(tmp_path / "a", flags, _opt(nonfinite="skip", max_consecutive_skips=2))
    assert code == 1 and tr.steps == 6
    assert tr.saves == [("latest", 3), ("best", 3)]  # nothing after the streak was seen
    assert open(tmp_path / "a" / "latest.pth").read() == "3"
    assert log[-1] == {"type": "skip_limit", "step": 4, "epoch": 0, "iter": 4, "consecutive": 3}
    assert "step 4" in lines[-1] and "3 consecutive" in lines[-1]
    assert [r["step"] for r in log if r["type"] == "skipped"] == [4, 5, 6]
    # a streak as long as the limit is tolerated
    code, tr, log, _ = _fit(tmp_path / "b", flags, _opt(nonfinite="skip", max_consecutive_skips=4))
    assert code == 0 and tr.steps == 10
    assert [r for r in log if r["type"] == "train"][-1]["skipped_total"] == 4
    # the default limit is 10
    flags = {i: GRAD for i in range(0, 10)}
    code, tr, log, _ = _fit(tmp_path / "c", flags, _opt(nonfinite="skip", valid_freq=50, epoch=4))
    assert code == 0 and tr.steps == 20
    flags = {i: GRAD for i in range(0, 11)}
    code, tr, log, _ = _fit(tmp_path / "d", flags, _opt(nonfinite="skip", valid_freq=50, epoch=4))
    assert code == 1 and tr.steps == 12 and tr.saves == []
    assert log[-1]["type"] == "skip_limit" and log[-1]["step"] == 1 and log[-1]["consecutive"] == 11


def test_fit_skip_mode_refuses_to_checkpoint_a_nonfinite_model(tmp_path):
    code, tr, log, lines = _fit(tmp_path / "a", {}, _opt(nonfinite="skip"), norm=float("nan"))
    assert code == 1 and tr.steps == 3 and tr.saves == []
    assert log[-1]["type"] == "nonfinite" and log[-1]["step"] == 3 and "parameter norm" in log[-1]["what"]
    assert not (tmp_path / "a" / "latest.pth").exists()
    assert "no checkpoint written" in lines[-1]
    code, tr, log, lines = _fit(tmp_path / "b", {}, _opt(nonfinite="skip"), buffers_ok=False)
    assert code == 1 and tr.saves == [] and "buffer" in log[-1]["what"]
    # under the default policy fit does not ask (today's behaviour)
    code, tr, log, _ = _fit(tmp_path / "c", {}, _opt(), buffers_ok=False)
    assert code == 0 and len(tr.saves) > 0


def test_fit_cross_checks_the_records_with_the_guard_state(tmp_path):
    tel = FakeTelemetry({1: GRAD})
    tr = FakeTrainer(tel)
    tr.optimizer.skipped_steps = lambda: (0, 0)  # the device says nothing was skipped
    with pytest.raises(RuntimeError, match="guard state"):
        fit(tr, iter([[("img", "gt")]] * 100), lambda: {"abs_rel": 0.5}, _opt(nonfinite="skip"), str(tmp_path),
            steps_per_epoch=5, log=lambda s: None)


def test_fit_skip_mode_needs_the_guarded_optimizer(tmp_path):
    tr = FakeTrainer(FakeTelemetry({}))

    class Unguarded:
        def param_norm(self):
            return torch.tensor(3.0)

    tr.optimizer = Unguarded()  # its update would have written the NaNs: nothing may be called "skipped"
    with pytest.raises(ValueError, match="skip_nonfinite"):
        fit(tr, iter([[("img", "gt")]] * 10), lambda: {"abs_rel": 0.5}, _opt(nonfinite="skip"), str(tmp_path),
            steps_per_epoch=5, log=lambda s: None)
    assert tr.steps == 0


# ---------------------------------------------------------------- config and CLI
def test_config_validation():
    from mdemi.train.builder import build_from_config, nonfinite_policy
    assert nonfinite_policy({}) == ("stop", 10)
    assert nonfinite_policy({"train": {"nonfinite": "skip", "max_consecutive_skips": 3}}) == ("skip", 3)
    for bad in ("Skip", "ignore", None, 1):
        with pytest.raises(ValueError, match="train.nonfinite"):
            nonfinite_policy({"train": {"nonfinite": bad}})
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="max_consecutive_skips"):
            nonfinite_policy({"train": {"max_consecutive_skips": bad}})
    cfg = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
           "dataloader": {"batch_size": 2}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1, "nonfinite": "skip"},
           "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001}}
    t = build_from_config(cfg, device="meta")
    assert t.optimizer.skip_nonfinite is True
    cfg["train"]["nonfinite"] = "stop"
    assert build_from_config(cfg, device="meta").optimizer.skip_nonfinite is False
    del cfg["train"]["nonfinite"]
    assert build_from_config(cfg, device="meta").optimizer.skip_nonfinite is False
    cfg["train"]["nonfinite"] = "drop"
    with pytest.raises(ValueError, match="train.nonfinite"):
        build_from_config(cfg, device="meta")


def test_cli_nonfinite_flag(tmp_path):
    from mdemi import run
    assert run._args(["--opt", "x"]).nonfinite is None
    assert run._args(["--opt", "x", "--nonfinite", "skip"]).nonfinite == "skip"
    with pytest.raises(SystemExit):
        run._args(["--opt", "x", "--nonfinite", "ignore"])
    # a bad config value is refused before anything else is set up
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "",
           "model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}, "optimizer": {"lr": 1e-4},
           "train": {"epoch": 1, "nonfinite": "carry-on"}, "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    try:
        with pytest.raises(ValueError, match="train.nonfinite"):
            run.main(["--opt", str(path), "--test"])
    finally:  # parse() exports the config's gpu_ids
        if env is None:
            os.environ.pop("HIP_VISIBLE_DEVICES", None)
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = env


# ---------------------------------------------------------------- Telemetry.drain on a hand-made ring
def test_drain_returns_flagged_records_when_asked():
    tel = Telemetry(capacity=4, device="cpu")
    raw = tel._buf.numpy()  # [state | 4 records], shares the buffer
    ring = raw[16:].view(np.dtype([("loss", "<f4"), ("grad_sumsq", "<f4"), ("index", "<i4"), ("flags", "<u4")]))
    # five pushes into four slots: record 4 overwrote record 0; 2 was skipped, 3 had a NaN loss only
    for i, (lo, gs, fl) in {1: (2.0, 1.0, 0), 2: (math.nan, math.inf, GRAD | LOSS), 3: (math.nan, 0.5, LOSS),
                            4: (5.0, 0.25, 0)}.items():
        ring[i % 4] = (lo, gs, i, fl)
    raw[:16].view("<i4")[:] = [5, 2, 2, 0]
    with pytest.raises(NonFiniteStep) as e:
        tel.drain()
    assert e.value.first_index == 2 and e.value.count == 2
    d = tel.drain(raise_on_nonfinite=False)
    assert d.pushed == 5 and d.dropped == 1
    assert [(r.index, r.flags) for r in d.records] == [(1, 0), (2, GRAD | LOSS), (3, LOSS), (4, 0)]
    assert math.isinf(d.records[1].grad_sumsq) and d.records[3].loss == 5.0
    assert tel.drain(raise_on_nonfinite=False).records == []  # the position advanced
    with pytest.raises(NonFiniteStep):  # the default still raises: the device counter is cumulative
        tel.drain()


# ---------------------------------------------------------------- schedule_step in the optimizer state
def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(4))]


def _with_state(opt, ps, steps, step_count):
    for p in ps:
        opt.state[p] = {"exp_avg": torch.full_like(p, 0.5), "exp_avg_sq": torch.full_like(p, 0.25)}
    opt.steps, opt.step_count = list(steps), step_count


def test_schedule_step_round_trip():
    from mdemi.train import FusedAdamW
    from mdemi.train.optim import schedule_position
    ps = _params()
    opt = FusedAdamW(ps, lr=1e-3, skip_nonfinite=True)
    _with_state(opt, ps, [4, 4], 6)  # two of six steps were skipped
    sd = opt.state_dict()
    assert sd["schedule_step"] == 6
    assert [float(sd["state"][i]["step"]) for i in (0, 1)] == [4.0, 4.0]
    qs = _params()
    opt2 = FusedAdamW(qs, lr=1e-3, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 6 and opt2.steps == [4, 4]
    # the unguarded optimizer reads the key too (a run resumed under the default policy)
    opt3 = FusedAdamW(_params(), lr=1e-3)
    opt3.load_state_dict(sd)
    assert opt3.step_count == 6 and opt3.steps == [4, 4]
    # torch's loader ignores the extra top-level key
    ref = torch.optim.AdamW(_params(), lr=1e-3)
    ref.load_state_dict(sd)
    assert [float(ref.state[p]["step"]) for p in ref.param_groups[0]["params"]] == [4.0, 4.0]
    # the file format survives torch.save / weights_only load
    assert schedule_position({"schedule_step": 6}, [4, 4]) == 6
    with pytest.raises(ValueError, match="schedule_step"):
        schedule_position({"schedule_step": 3}, [4, 4])


def test_state_without_schedule_step_loads_as_before():
    from mdemi.train import FusedAdamW
    from mdemi.train.optim import schedule_position
    ps = _params()
    opt = FusedAdamW(ps, lr=1e-3)  # the default optimizer writes no such key
    _with_state(opt, ps, [2, 5], 5)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    for skip in (False, True):
        o = FusedAdamW(_params(), lr=1e-3, skip_nonfinite=skip)
        o.load_state_dict(sd)
        assert o.step_count == 5 and o.steps == [2, 5]
    assert schedule_position({}, [2, 5]) == 5 and schedule_position({}, []) == 0
