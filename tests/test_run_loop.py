"""The training driver's host logic (mdemi.train.loop, mdemi.train.telemetry.decode_ring,
mdemi.run's argument checks, utils.common_utils.compute_param_norm) without a GPU."""
import json
import math
import os

import pytest
import torch

from mdemi.train.builder import optimizer_steps_per_epoch
from mdemi.train.loop import EpochStream, fit, step_rng
from mdemi.train.telemetry import Drained, NonFiniteStep, StepRecord, decode_ring

N, BATCH, WORLD, EPOCHS = 10, 2, 2, 3


def _streams(num_accum, **kw):
    return [EpochStream(N, BATCH, WORLD, r, seed=5, epochs=EPOCHS, num_accum=num_accum, **kw) for r in range(WORLD)]


@pytest.mark.parametrize("num_accum", [1, 2])
def test_epoch_stream_length_and_full_batches(num_accum):
    opt = {"dataloader": {"batch_size": BATCH}, "train": {"num_accum": num_accum}}
    per_epoch = optimizer_steps_per_epoch(opt, WORLD, images=N) * num_accum
    for s in _streams(num_accum):
        got = list(s)
        assert len(got) == len(s) == per_epoch * EPOCHS
        assert all(len(b) == BATCH and all(0 <= i < N for i in b) for b in got)
        for e in range(EPOCHS):
            assert got[e * per_epoch:(e + 1) * per_epoch] == s.epoch_batches(e)


def test_epoch_stream_ranks_disjoint_and_cover():
    a, b = _streams(1)
    for e in range(EPOCHS):
        ia = {i for bt in a.epoch_batches(e) for i in bt}
        ib = {i for bt in b.epoch_batches(e) for i in bt}
        assert not (ia & ib)
        assert ia | ib == set(range(N))


def test_epoch_stream_is_a_function_of_seed_and_epoch():
    a = _streams(1)[0]
    again = EpochStream(N, BATCH, WORLD, 0, seed=5, epochs=EPOCHS)
    assert list(a) == list(again)
    assert a.epoch_batches(0) != a.epoch_batches(1) != a.epoch_batches(2)
    # seed + epoch names the permutation
    assert EpochStream(N, BATCH, WORLD, 0, seed=6, epochs=1).epoch_batches(0) == a.epoch_batches(1)
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5)).tolist()
    padded = (order + order)[:12]
    assert a.epoch_batches(0) == [padded[0::2][i:i + 2] for i in (0, 2, 4)]


@pytest.mark.parametrize("num_accum", [1, 2])
def test_epoch_stream_start_yields_the_tail(num_accum):
    full = list(_streams(num_accum)[1])
    s = _streams(num_accum, start_epoch=1, start_step=2 if num_accum == 1 else 1)[1]
    per_epoch = s.batches_per_epoch
    skip = per_epoch + (2 if num_accum == 1 else 1) * num_accum
    assert list(s) == full[skip:]
    assert len(s) == len(full) - skip
    if num_accum == 1:
        assert skip == 5


def test_step_rng_is_a_function_of_its_arguments():
    from mdemi.dataset import GpuSampleTransform
    tf = GpuSampleTransform("NYU", "train", (416, 544))

    def draw(*key):
        return tf.draw(2, (480, 640), step_rng(*key))

    base = (3, 1, 7, 0, 0)
    assert draw(*base) == draw(*base)
    for pos in range(5):
        other = list(base)
        other[pos] += 1
        assert draw(*other) != draw(*base), pos


def _ring(capacity, pushed):
    """What the device ring holds after `pushed` pushes."""
    slots = [StepRecord(0.0, 0.0, -1, 0)] * capacity
    for i in range(pushed):
        slots[i % capacity] = StepRecord(float(i + 1), float(i), i, 0)
    return slots


def test_decode_ring():
    recs, dropped = decode_ring(_ring(4, 3), pushed=3, last_seen=0, capacity=4)
    assert [r.index for r in recs] == [0, 1, 2] and dropped == 0
    recs, dropped = decode_ring(_ring(4, 6), pushed=6, last_seen=0, capacity=4)
    assert [r.index for r in recs] == [2, 3, 4, 5] and dropped == 2
    assert [r.loss for r in recs] == [3.0, 4.0, 5.0, 6.0]
    recs, dropped = decode_ring(_ring(4, 6), pushed=6, last_seen=6, capacity=4)
    assert recs == [] and dropped == 0
    # a partial window that wraps the ring
    recs, dropped = decode_ring(_ring(4, 6), pushed=6, last_seen=3, capacity=4)
    assert [r.index for r in recs] == [3, 4, 5] and dropped == 0
    # dict records (and numpy records) are read by key
    recs, _ = decode_ring([{"index": 4}, {"index": 5}, {"index": 2}, {"index": 3}], 6, 4, 4)
    assert [r["index"] for r in recs] == [4, 5]
    with pytest.raises(ValueError):
        decode_ring(_ring(4, 6), pushed=5, last_seen=6, capacity=4)
    with pytest.raises(ValueError):
        decode_ring(_ring(4, 2), pushed=6, last_seen=0, capacity=4)  # slots do not hold what pushed says


# ---------------------------------------------------------------- fit with fakes
class FakeTelemetry:
    def __init__(self, bad_at=None):
        self.records, self.seen, self.bad_at = [], 0, bad_at

    def push(self, loss):
        self.records.append(StepRecord(loss, 4.0, len(self.records), 0))

    def drain(self):
        if self.bad_at is not None and len(self.records) > self.bad_at:
            raise NonFiniteStep(self.bad_at)
        new = self.records[self.seen:]
        self.seen = len(self.records)
        return Drained(new, 0, self.seen)


class FakeOptimizer:
    def param_norm(self):
        return torch.tensor(3.0)


class FakeScheduler:
    def get_last_lr(self):
        return [1e-5, 1e-4]


class FakeTrainer:
    def __init__(self, telemetry):
        self.telemetry, self.optimizer, self.scheduler = telemetry, FakeOptimizer(), FakeScheduler()
        self.epoch, self.steps, self.saves = 0, 0, []

    def step(self, batches):
        self.steps += 1
        self.telemetry.push(float(self.steps))

    def save(self, prefix, save_dir, current_iter, best_value, best_epoch=None, best_iter=None, model_only=False):
        self.saves.append((prefix, self.steps, self.epoch, current_iter, best_value, best_epoch, best_iter))
        with open(os.path.join(save_dir, prefix + ".pth"), "w") as f:
            f.write(str(self.steps))


OPT = {"dataloader": {"batch_size": 2}, "train": {"print_freq": 2, "valid_freq": 3, "epoch": 2, "num_accum": 1}}


def _fit(tmp_path, abs_rels, **kw):
    tel = FakeTelemetry(kw.pop("bad_at", None))
    tr = FakeTrainer(tel)
    vals = iter(abs_rels)
    lines = []
    code = fit(tr, iter([[("img", "gt")]] * 100), lambda: {"abs_rel": next(vals), "rmse": 1.0}, OPT, str(tmp_path),
               steps_per_epoch=5, log=lines.append, **kw)
    log = [json.loads(s) for s in open(tmp_path / "log.jsonl")] if (tmp_path / "log.jsonl").exists() else []
    return code, tr, log, lines


def test_fit_cadence_and_best_checkpoint(tmp_path):
    code, tr, log, lines = _fit(tmp_path, [0.5, 0.6, 0.4, 0.45])
    assert code == 0 and tr.steps == 10
    train = [r for r in log if r["type"] == "train"]
    valid = [r for r in log if r["type"] == "valid"]
    assert [r["step"] for r in train] == [2, 4, 6, 8, 10]
    assert [(r["epoch"], r["iter"]) for r in train] == [(0, 2), (0, 4), (1, 1), (1, 3), (1, 5)]
    assert [r["loss"] for r in train] == [1.5, 3.5, 5.5, 7.5, 9.5]  # the window's mean
    for r in train:
        assert r["grad_norm"] == r["grad_norm_max"] == 2.0 and r["param_norm"] == 3.0 and r["lr"] == 1e-4
        assert r["dropped"] == 0 and r["images_per_sec"] > 0
        assert set(r) == {"type", "epoch", "iter", "step", "loss", "grad_norm", "grad_norm_max", "param_norm", "lr",
                          "images_per_sec", "dropped"}
    # every valid_freq steps and at the end of the last epoch
    assert [r["step"] for r in valid] == [3, 6, 9, 10]
    assert [r["best"] for r in valid] == [True, False, True, False]
    assert [(p, s) for p, s, *_ in tr.saves] == [("latest", 3), ("best", 3), ("latest", 6), ("latest", 9), ("best", 9),
                                                 ("latest", 10)]
    # (prefix, steps, epoch, iter, best value, best epoch, best iter)
    assert tr.saves[2] == ("latest", 6, 1, 1, 0.5, 0, 3)
    assert tr.saves[-1] == ("latest", 10, 1, 5, 0.4, 1, 4)
    assert len(lines) == len(log)


def test_fit_max_steps_and_resume_position(tmp_path):
    code, tr, log, _ = _fit(tmp_path, [0.5], max_steps=4)
    assert code == 0 and tr.steps == 4
    assert [(r["type"], r["step"]) for r in log] == [("train", 2), ("valid", 3), ("train", 4)]
    assert tr.saves[-1][:4] == ("latest", 4, 0, 4)  # a resumable state where the run stopped
    # the continuation: global steps 5..10
    code, tr2, log2, _ = _fit(tmp_path, [0.7, 0.3, 0.2], start_epoch=0, start_step=4, max_steps=None,
                              best=(0.5, 0, 3))
    assert code == 0 and tr2.steps == 6
    assert [(r["type"], r["step"]) for r in log2[len(log):]] == [("train", 6), ("valid", 6), ("train", 8), ("valid", 9),
                                                                 ("train", 10), ("valid", 10)]
    assert [r["best"] for r in log2 if r["type"] == "valid"][1:] == [False, True, True]


def test_fit_stops_on_nonfinite_step_without_a_checkpoint(tmp_path):
    # record 4 (global step 5) is flagged: the drain at step 6 raises, before validation 6 saves
    code, tr, log, lines = _fit(tmp_path, [0.5, 0.1], bad_at=4)
    assert code != 0
    assert tr.steps == 6
    assert [(p, s) for p, s, *_ in tr.saves] == [("latest", 3), ("best", 3)]
    assert open(tmp_path / "latest.pth").read() == "3"
    assert log[-1] == {"type": "nonfinite", "step": 5, "epoch": 0, "iter": 5, "count": 1}
    assert "step 5" in lines[-1]


# ---------------------------------------------------------------- CLI and utilities
def test_cli_test_mode_needs_a_checkpoint(tmp_path):
    from mdemi import run
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "",
           "model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1},
           "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    try:
        with pytest.raises(SystemExit) as e:
            run.main(["--opt", str(path), "--test"])
        assert "checkpoint" in str(e.value) and "missing" in str(e.value)
        with pytest.raises(SystemExit) as e:
            run.main(["--opt", str(path), "--test", "--checkpoint", str(tmp_path / "nope.pth")])
        assert "nope.pth" in str(e.value)
    finally:  # parse() exports the config's gpu_ids
        if env is None:
            os.environ.pop("HIP_VISIBLE_DEVICES", None)
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = env


def test_compute_param_norm_cpu():
    from mdemi.utils.common_utils import compute_param_norm
    g = torch.Generator().manual_seed(0)
    ps = [torch.randn(7, 5, generator=g, requires_grad=True), torch.randn(33, generator=g, requires_grad=True),
          torch.randn(4, generator=g)]  # the last one does not require grad: not counted
    # the reference formula: the p-norm of the per-parameter p-norms over requires_grad parameters
    for p in (2.0, 1.0, 3.0):
        want = sum(float(t.detach().abs().double().pow(p).sum()) for t in ps[:2]) ** (1.0 / p)
        got = compute_param_norm(ps, p)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
        assert math.isclose(got.item(), want, rel_tol=1e-5)
    assert compute_param_norm(ps[0]).item() == pytest.approx(ps[0].detach().norm().item(), rel=1e-6)
    zero = compute_param_norm([ps[2]])
    assert isinstance(zero, torch.Tensor) and zero.item() == 0.0


def test_common_utils_small_helpers(capsys):
    from mdemi.utils.common_utils import Timer, dprint, time_log, zero_grad_bn
    dprint("a", 1, local_rank=0)
    dprint("hidden", local_rank=1)
    assert capsys.readouterr().out == "a 1\n"
    s = time_log()
    assert s.startswith("*" * 48 + "  ") and s.endswith("\n") and "|" in s
    t = Timer()
    assert t.update() >= 0.0
    m = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 1), torch.nn.BatchNorm2d(2))
    m(torch.randn(2, 1, 3, 3)).sum().backward()
    zero_grad_bn(m)
    assert m[0].weight.grad is not None and all(p.grad is None for p in m[1].parameters())
