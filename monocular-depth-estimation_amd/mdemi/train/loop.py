"""The restated run.py's loop: epochs of file batches into Trainer.step, a log line every
train.print_freq optimizer steps read from the device telemetry ring, validation and
checkpoints every train.valid_freq steps.

The reference's run.py is absent from the snapshot; the traceback in
output/test/wandb/latest-run/run-1pklfwui.wandb shows ``for i, data in
enumerate(train_loader)`` and the configs name print_freq / valid_freq / epoch.  What is
parity and what is a decision is listed in DESIGN.md §1c.  In short:

  EpochStream   every remaining epoch as one batch-sampler stream (DataLoader workers start
                once); epoch e is the permutation of torch.Generator().manual_seed(seed + e),
                wrapped to full batches and sharded rank::world (DistributedSampler's layout)
  step_rng      the augmentation draws of one micro-batch: a fresh random.Random per
                (seed, epoch, step, micro, rank), so the data of any step is a pure function of
                where the step is -- a resumed run continues the identical stream
  fit           the loop; one host synchronisation per print_freq steps (Telemetry.drain)

train.nonfinite "skip": the guarded optimizer step has already dropped a step whose gradient
sum of squares was not finite (the record's MDEMI_STEP_GRAD_NONFINITE flag is that same
predicate), so fit counts such records instead of stopping.  A skipped step is still a step:
the schedule, the epoch stream and step_rng are functions of the step index and advance;
only the weights, the moments and the bias-correction counts stand still.
"""
from __future__ import annotations

import json
import math
import os
import random
import time

import torch

from .. import _lib as L
from ..utils.dist_utils import all_reduce_dict
from .builder import (eval_align, eval_boundary, eval_record, eval_tile, nonfinite_policy,
                      optimizer_steps_per_epoch)
from .ema import ema_config
from .telemetry import NonFiniteStep

LOG_NAME = "log.jsonl"


def step_rng(seed, epoch, step, micro, rank):
    """The random.Random that draws one micro-batch's augmentation parameters
    (GpuSampleTransform(..., rnd=...))."""
    return random.Random(f"mdemi/{int(seed)}/{int(epoch)}/{int(step)}/{int(micro)}/{int(rank)}")


class EpochStream(torch.utils.data.Sampler):
    """Batch sampler over epochs start_epoch .. epochs-1 as one stream of index lists.

    Per epoch and rank it yields optimizer_steps_per_epoch(opt, world, images=n) * num_accum
    batches of exactly ``batch`` indices: the epoch's permutation is wrapped around to
    ceil(n / (batch * world)) * batch * world indices, sharded rank::world and cut into
    batches; the trailing batches that do not fill an optimizer step are dropped (and a
    dataset shorter than one step wraps further), so the count is the one build_scheduler
    sized the OneCycle schedule with.  start_step skips that many optimizer steps of
    start_epoch: the stream is exactly the tail of the full one."""

    def __init__(self, n, batch, world=1, rank=0, seed=0, epochs=1, num_accum=1, start_epoch=0, start_step=0):
        if n <= 0 or batch <= 0 or world <= 0 or not 0 <= rank < world or num_accum <= 0:
            raise ValueError(f"EpochStream: bad arguments n={n} batch={batch} world={world} rank={rank} "
                             f"num_accum={num_accum}")
        self.n, self.batch, self.world, self.rank = int(n), int(batch), int(world), int(rank)
        self.seed, self.epochs, self.num_accum = int(seed), int(epochs), int(num_accum)
        self.steps_per_epoch = optimizer_steps_per_epoch(
            {"dataloader": {"batch_size": self.batch}, "train": {"num_accum": self.num_accum}}, self.world,
            images=self.n)
        self.batches_per_epoch = self.steps_per_epoch * self.num_accum
        if not (0 <= start_epoch <= self.epochs and 0 <= start_step <= self.steps_per_epoch):
            raise ValueError(f"EpochStream: start ({start_epoch}, {start_step}) outside {self.epochs} epochs of "
                             f"{self.steps_per_epoch} steps")
        self.start_epoch, self.start_step = int(start_epoch), int(start_step)

    def epoch_batches(self, epoch):
        """This rank's batches (index lists) of one epoch."""
        order = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed + epoch)).tolist()
        group = self.batch * self.world
        total = max(math.ceil(self.n / group), self.batches_per_epoch) * group
        padded = (order * math.ceil(total / self.n))[:total]
        mine = padded[self.rank::self.world]
        return [mine[i * self.batch:(i + 1) * self.batch] for i in range(self.batches_per_epoch)]

    def __iter__(self):
        for e in range(self.start_epoch, self.epochs):
            skip = self.start_step * self.num_accum if e == self.start_epoch else 0
            yield from self.epoch_batches(e)[skip:]

    def __len__(self):
        left = (self.epochs - self.start_epoch) * self.batches_per_epoch - self.start_step * self.num_accum
        return max(0, left)


class TrainBatches:
    """Decoded loader batches -> the micro-batch lists Trainer.step takes: num_accum loader
    batches per optimizer step, each through the GPU sample transform with its own
    step_rng."""

    def __init__(self, loader_iter, transform, num_accum, steps_per_epoch, seed=0, rank=0, start_epoch=0,
                 start_step=0):
        self.it, self.tf, self.num_accum, self.spe = loader_iter, transform, int(num_accum), int(steps_per_epoch)
        self.seed, self.rank = seed, rank
        self.epoch, self.step = divmod(start_epoch * self.spe + start_step, self.spe)

    def __iter__(self):
        return self

    def __next__(self):
        micro = []
        for m in range(self.num_accum):
            b = next(self.it)  # StopIteration ends the stream
            img, gt, _ = self.tf(b["image"], b["depth"], rnd=step_rng(self.seed, self.epoch, self.step, m, self.rank))
            micro.append((img, gt))
        self.epoch, self.step = divmod(self.epoch * self.spe + self.step + 1, self.spe)
        return micro


def _finite_mean(vals):
    return sum(vals) / len(vals) if vals else None


class _Stop(Exception):
    """fit's skip mode gives up: ``rec`` goes to log.jsonl, ``msg`` to the log."""

    def __init__(self, rec, msg):
        super().__init__(msg)
        self.rec, self.msg = rec, msg


def _append(path, rec):
    with open(path, "a", encoding="utf-8") as f:
        f.write(json.dumps(rec) + "\n")


def fit(trainer, train_batches, validate, opt, out_dir, *, telemetry=None, steps_per_epoch=None, start_epoch=0,
        start_step=0, max_steps=None, rank=0, world=1, best=None, log=print):
    """Run the train loop; returns the process exit code (0, or 1 after a non-finite step).

    train.nonfinite "skip" (the trainer's optimizer is FusedAdamW(skip_nonfinite=True)): a
    record flagged GRAD_NONFINITE is a step the device dropped -- logged as {"type":
    "skipped", step, epoch, iter}, counted in the train record's "skipped" (window) and
    "skipped_total" and kept out of its means; one flagged LOSS_NONFINITE only was applied
    with a finite gradient and is logged as {"type": "nonfinite_loss", ...}.  The run ends
    with exit code 1 when more than train.max_consecutive_skips steps in a row were skipped,
    or when a checkpoint is due and the parameter norm or a floating-point buffer of the
    model is not finite (nothing is written then, as under "stop").

    train_batches yields one list of train.num_accum (image, gt) micro-batches per optimizer
    step, starting at (start_epoch, start_step); validate() returns the metric dict
    (evaluate(..., weight_by_count=True)) and is called on every rank.  With averaged weights
    (trainer.ema, train.ema_decay) it is called as validate(model) instead: on trainer.ema.module
    after ModelEma.sync_buffers -- the "valid" record then carries "weights": "ema" and best.pth
    is chosen on its abs_rel -- and, under train.ema_validate "both", on trainer.model too, for
    a second record with "weights": "model".  With eval.align other than "none" the caller's
    validate() reports aligned metrics; the record then carries "align": MODE and best.pth is
    chosen on the aligned abs_rel.  With eval.tile the caller's validate() predicts in tiles and the
    record carries "tile": [h, w] and "tile_align".  With eval.boundary it reports the boundary
    scores too; the records (the raw weights' one under "both" included) then carry them,
    "boundary_images" and "boundary": [t_min, t_max, n]; best.pth is still chosen on abs_rel.
    telemetry defaults to
    trainer.telemetry.  ``best`` is (abs_rel, epoch, iter) of the best checkpoint so far
    (a resumed run).  Rank 0 writes out_dir/log.jsonl -- {"type": "train", ...} every
    train.print_freq steps, {"type": "valid", ...} per validation -- and latest.pth /
    best.pth through Trainer.save."""
    tr = opt.get("train", {})
    print_freq = max(1, int(tr.get("print_freq", 20)))
    valid_freq = max(1, int(tr.get("valid_freq", 500)))
    epochs = int(tr.get("epoch", 1))
    num_accum = int(tr.get("num_accum", 1))
    batch = int(opt.get("dataloader", {}).get("batch_size", 8))
    spe = int(steps_per_epoch) if steps_per_epoch is not None else optimizer_steps_per_epoch(opt, world)
    total = epochs * spe
    stop = total if max_steps is None else min(total, int(max_steps))
    telemetry = telemetry if telemetry is not None else getattr(trainer, "telemetry", None)
    if telemetry is None:
        raise ValueError("fit: needs a Telemetry (Trainer(..., telemetry=...))")
    log_path = os.path.join(out_dir, LOG_NAME)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
    best_value, best_epoch, best_iter = best if best is not None else (math.inf, None, None)

    # averaged weights (train.ema_decay): validate(model) is then called with the model to
    # evaluate -- trainer.ema.module, and trainer.model as well under train.ema_validate "both"
    ema = getattr(trainer, "ema", None)
    ema_validate = ema_config(opt)[2]

    policy, max_skips = nonfinite_policy(opt)
    align = eval_align(opt)
    tile = eval_tile(opt)
    boundary = eval_boundary(opt)
    skip_mode = policy == "skip"
    guard = getattr(trainer.optimizer, "skipped_steps", None) if skip_mode else None
    if skip_mode and (guard is None or not getattr(trainer.optimizer, "skip_nonfinite", True)):
        # without the guarded update a flagged step HAS written its NaNs: never count it as skipped
        raise ValueError('fit: train.nonfinite "skip" needs an optimizer with the guarded step '
                         "(FusedAdamW(skip_nonfinite=True); build_from_config passes it)")

    done = start_epoch * spe + start_step  # optimizer steps completed (the global step)
    base = done  # telemetry record i is global step base + i + 1
    window, dropped = [], 0
    # skip mode: steps skipped in the window / in this call, the current streak of skipped
    # steps and the global step it began at, and the optimizer's counters when fit began
    w_skipped = skipped_total = 0
    skipped0, streak = guard() if guard is not None else (0, 0)
    streak_first = base - streak + 1
    t_window, n_window = time.perf_counter(), 0
    validated_at = None
    lr_used = None

    def where(gstep):
        e, s = divmod(gstep - 1, spe)
        return {"step": gstep, "epoch": e, "iter": s + 1}

    def drain():
        nonlocal dropped, w_skipped, skipped_total, streak, streak_first
        if not skip_mode:
            d = telemetry.drain()
            window.extend(d.records)
            dropped += d.dropped
            return
        d = telemetry.drain(raise_on_nonfinite=False)
        dropped += d.dropped
        lines, over = [], None  # over: (first step, length) of a streak beyond the limit
        for r in d.records:
            gstep = base + r.index + 1
            if r.flags & L.STEP_GRAD_NONFINITE:
                w_skipped += 1
                skipped_total += 1
                streak += 1
                if streak == 1:
                    streak_first = gstep
                if streak > max_skips:
                    over = (streak_first, streak)
                lines.append({"type": "skipped", **where(gstep)})
                continue
            streak = 0
            if r.flags & L.STEP_LOSS_NONFINITE:
                lines.append({"type": "nonfinite_loss", **where(gstep)})
            window.append(r)
        if guard is not None:
            # the optimizer's own counters (mdemi_guard_state), read at the same point: they
            # must tell the same story as the records; when the ring overflowed they stand in
            dev_skipped, dev_streak = guard()
            if d.dropped:
                skipped_total, streak = dev_skipped - skipped0, dev_streak
                streak_first = done - streak + 1
                if streak > max_skips:
                    over = (streak_first, streak)
            elif (dev_skipped - skipped0, dev_streak) != (skipped_total, streak):
                raise RuntimeError(f"fit: the telemetry records count {skipped_total} skipped step(s), streak "
                                   f"{streak}; the optimizer's guard state says {dev_skipped - skipped0}, streak "
                                   f"{dev_streak}")
        if rank == 0:
            for rec in lines:
                _append(log_path, rec)
                log(json.dumps(rec))
        if over is not None:
            first, n = over
            raise _Stop({"type": "skip_limit", **where(first), "consecutive": n},
                        f"{n} consecutive optimizer steps skipped for non-finite gradients, the first at step "
                        f"{first} (epoch {where(first)['epoch']}, iter {where(first)['iter']}); "
                        f"train.max_consecutive_skips is {max_skips}: no checkpoint written, stopping.")

    def require_finite_model():
        """Skip mode, before a checkpoint: the rule 'never checkpoint a non-finite model' for
        what the guarded step cannot cover (BatchNorm running statistics written by a forward
        that overflowed).  Buffers are rank-local, so the verdict is reduced over the ranks."""
        pn = trainer.optimizer.param_norm()
        bad_norm = not math.isfinite(float(pn.item() if hasattr(pn, "item") else pn))
        ok_buffers = getattr(trainer, "buffers_finite", None)
        bad_buf = ok_buffers is not None and not ok_buffers()
        red = all_reduce_dict({"norm": float(bad_norm), "buffers": float(bad_buf)}, op="mean")
        if red["norm"] > 0 or red["buffers"] > 0:
            what = "parameter norm" if red["norm"] > 0 else "model buffer (BatchNorm running statistics)"
            raise _Stop({"type": "nonfinite", **where(done), "count": 0, "what": what},
                        f"non-finite {what} at optimizer step {done} with a checkpoint due: no checkpoint written, "
                        "stopping.")

    def emit_train(epoch, it):
        nonlocal window, dropped, t_window, n_window, w_skipped
        now = time.perf_counter()
        losses = [r.loss for r in window if not r.flags & L.STEP_LOSS_NONFINITE]
        norms = [math.sqrt(r.grad_sumsq) for r in window if r.grad_sumsq >= 0]
        rate = n_window * batch * num_accum / max(now - t_window, 1e-9)
        red = all_reduce_dict({"loss": float(_finite_mean(losses) or 0.0), "images_per_sec": float(rate)}, op="mean")
        pn = trainer.optimizer.param_norm()
        rec = {"type": "train", "epoch": epoch, "iter": it, "step": done, "loss": red["loss"],
               "grad_norm": _finite_mean(norms), "grad_norm_max": max(norms) if norms else None,
               "param_norm": float(pn.item() if hasattr(pn, "item") else pn),
               "lr": lr_used,
               "images_per_sec": red["images_per_sec"] * world, "dropped": dropped}
        if skip_mode:
            rec.update(skipped=w_skipped, skipped_total=skipped_total)
            w_skipped = 0
        if rank == 0:
            _append(log_path, rec)
            log(json.dumps(rec))
        window, dropped, t_window, n_window = [], 0, time.perf_counter(), 0

    def run_validation(epoch, it):
        nonlocal best_value, best_epoch, best_iter, validated_at, t_window
        t0 = time.perf_counter()
        if skip_mode:
            require_finite_model()
        raw = None
        if ema is None:
            metrics = eval_record(validate(), boundary)
        else:  # the averaged weights under the live model's current buffers
            ema.sync_buffers(trainer.model)
            metrics = eval_record(validate(ema.module), boundary)
            if ema_validate == "both":
                raw = eval_record(validate(trainer.model), boundary)
        if hasattr(trainer, "train_mode"):
            trainer.train_mode()  # evaluate() restores model.train(); frozen BatchNorms go back to eval
        improved = metrics["abs_rel"] < best_value
        if improved:
            best_value, best_epoch, best_iter = metrics["abs_rel"], epoch, it
        rec = {"type": "valid", "epoch": epoch, "iter": it, "step": done, **metrics, "best": improved}
        recs = [rec]
        if align != "none":  # the metrics, and so the choice of best.pth, are those of aligned predictions
            rec["align"] = align
            if raw is not None:
                raw["align"] = align
        if tile is not None:  # and those of predictions blended from tiles
            for r in (rec, raw):
                if r is not None:
                    r.update(tile=list(tile["tile"]), tile_align=tile["align"])
        if ema is not None:
            rec["weights"] = "ema"
            if raw is not None:  # for the record only: best.pth is chosen on the averaged weights
                recs.append({"type": "valid", "epoch": epoch, "iter": it, "step": done, **raw, "best": False,
                             "weights": "model"})
        if rank == 0:
            trainer.save("latest", out_dir, it, best_value, best_epoch=best_epoch, best_iter=best_iter)
            if improved:
                trainer.save("best", out_dir, it, best_value, best_epoch=best_epoch, best_iter=best_iter)
            for r in recs:
                _append(log_path, r)
                log(json.dumps(r))
        validated_at = done
        t_window += time.perf_counter() - t0  # validation time is not training throughput

    try:
        feed = iter(train_batches)
        while done < stop:
            batches = next(feed, None)
            if batches is None:
                break
            epoch, step = divmod(done, spe)
            if trainer.epoch != epoch or done == base:
                trainer.epoch = epoch
                if hasattr(trainer, "train_mode"):
                    trainer.train_mode()
            sched = getattr(trainer, "scheduler", None)
            lr_used = float(sched.get_last_lr()[-1]) if sched is not None else None  # this step's (last group)
            trainer.step(batches)
            done += 1
            n_window += 1
            it = step + 1  # optimizer steps completed in this epoch
            if done % print_freq == 0:
                drain()
                emit_train(epoch, it)
            if done % valid_freq == 0 or done == total:
                drain()  # a non-finite step must surface before its weights reach a checkpoint
                run_validation(epoch, it)
        if done > base and validated_at != done and done < total:
            # ended early (max_steps): leave a resumable latest.pth, without a validation
            drain()
            if skip_mode:
                require_finite_model()
            if rank == 0:
                epoch, step = divmod(done - 1, spe)
                trainer.epoch = epoch
                trainer.save("latest", out_dir, step + 1, best_value, best_epoch=best_epoch, best_iter=best_iter)
    except NonFiniteStep as e:
        bad = base + e.first_index + 1
        epoch, step = divmod(bad - 1, spe)
        msg = (f"non-finite loss or gradient norm at optimizer step {bad} (epoch {epoch}, iter {step + 1}); "
               f"{e.count} such step(s) recorded. The weights after it are not finite: no checkpoint written, "
               "stopping.")
        if rank == 0:
            _append(log_path, {"type": "nonfinite", "step": bad, "epoch": epoch, "iter": step + 1, "count": e.count})
        log(msg)
        return 1
    except _Stop as e:
        if rank == 0:
            _append(log_path, e.rec)
        log(e.msg)
        return 1
    return 0
