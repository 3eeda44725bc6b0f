"""python -m mdemi.run --opt CFG [--test]: train / validate / test from a reference config.

The reference's one entry point, ``run.py --opt cfg.json [--test]``, is missing from the
snapshot; the traceback in output/test/wandb/latest-run/run-1pklfwui.wandb shows
its call shape, ``run(parser_opt, is_test=parser_args.test, ...)``.  This driver reads the
same JSON configs unchanged (utils.common_utils.parse) and puts the existing pieces
together: DepthDataset + collate_raw in DataLoader workers, GpuSampleTransform,
build_from_config's Trainer, the device telemetry ring, evaluate and save_checkpoint
(train.loop.fit).  Training writes <output_dir>/log.jsonl, latest.pth and best.pth;
--test evaluates a checkpoint on the test split once.  Under torchrun (RANK / WORLD_SIZE /
LOCAL_RANK) it joins the "nccl" group; it does not launch ranks itself, and there is no
wandb.  Decisions are listed in DESIGN.md §1c.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

MAX_WORKERS = 15  # decoder processes per rank: with the main process, the 16 CPUs a job is given


def _args(argv):
    ap = argparse.ArgumentParser(prog="python -m mdemi.run", description=__doc__.split("\n\n")[0])
    ap.add_argument("--opt", required=True, help="the run's JSON config (the reference's format)")
    ap.add_argument("--test", action="store_true", help="evaluate the checkpoint on the test split and exit")
    ap.add_argument("--checkpoint", default=None, help="resume from / evaluate this file (default: the config's "
                                                       "\"checkpoint\" key)")
    ap.add_argument("--list-root", default=None, help="directory of the train_test_inputs file lists")
    ap.add_argument("--graph", action="store_true", help="capture the train step in a hipGraph")
    ap.add_argument("--precision", default=None, choices=["fp32", "fp32e", "bf16"])
    ap.add_argument("--drop-path", type=float, default=None, help="override the model's stochastic-depth rate")
    ap.add_argument("--seed", type=int, default=0, help="weight init, epoch permutations and augmentation draws")
    ap.add_argument("--nonfinite", default=None, choices=["stop", "skip"],
                    help="override the config's train.nonfinite: stop at a non-finite step (the default), or "
                         "skip its update on the device and go on")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="override the config's train.ema_decay: keep an exponential moving average of the "
                         "weights with this decay, validate it and choose best.pth on it")
    ap.add_argument("--grad-weight", type=float, default=None,
                    help="override the config's loss.grad_weight: add this weight times the multi-scale "
                         "gradient-matching loss to the training loss (0 switches the term off)")
    ap.add_argument("--ssi-weight", type=float, default=None,
                    help="override the config's loss.ssi_weight: add this weight times the scale- and "
                         "shift-invariant loss to the training loss (0 switches the term off)")
    ap.add_argument("--align", default=None, choices=["none", "median", "lstsq", "lstsq_disp"],
                    help="override the config's eval.align: align each prediction to its ground truth before the "
                         "metrics (validation and --test) by median scaling, or by least-squares scale and shift "
                         "in depth (lstsq) or in inverse depth (lstsq_disp)")
    ap.add_argument("--tile", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="override the config's eval.tile: validate / test on overlapping H x W tiles of each "
                         "image, blended back to its size")
    ap.add_argument("--tile-overlap", type=int, nargs="+", default=None, metavar="N",
                    help="override eval.tile_overlap: one overlap for both axes, or OY OX (default: a quarter of "
                         "the tile)")
    ap.add_argument("--tile-align", default=None, choices=["none", "lstsq", "lstsq_disp"],
                    help="override eval.tile_align: fit each tile's scale and shift to the tiles before it")
    ap.add_argument("--boundary", action="store_true",
                    help="set the config's eval.boundary: report the scale-invariant boundary F1, precision and "
                         "recall of the depth edges next to the nine metrics (validation and --test)")
    ap.add_argument("--ema", action="store_true",
                    help="with --test: evaluate the checkpoint's averaged weights (ema_state_dict)")
    ap.add_argument("--max-steps", type=int, default=None, help="stop after this many optimizer steps (in all)")
    return ap.parse_args(argv)


def _override(opt, args):
    """The command line's overrides of config keys, written into opt."""
    if args.nonfinite is not None:
        opt.setdefault("train", {})["nonfinite"] = args.nonfinite
    if args.ema_decay is not None:
        opt.setdefault("train", {})["ema_decay"] = args.ema_decay
    if args.grad_weight is not None:
        opt.setdefault("loss", {})["grad_weight"] = args.grad_weight
    if args.ssi_weight is not None:
        opt.setdefault("loss", {})["ssi_weight"] = args.ssi_weight
    if args.align is not None:
        opt.setdefault("eval", {})["align"] = args.align
    if args.boundary:
        opt.setdefault("eval", {})["boundary"] = True
    tile_overrides(opt, args)
    return opt


def tile_overrides(opt, args):
    """--tile / --tile-overlap / --tile-align written over the config's eval.tile* keys."""
    if args.tile is not None:
        opt.setdefault("eval", {})["tile"] = list(args.tile)
    if args.tile_overlap is not None:
        if len(args.tile_overlap) > 2:
            raise SystemExit("--tile-overlap takes one value or two (OY OX)")
        o = args.tile_overlap
        opt.setdefault("eval", {})["tile_overlap"] = o[0] if len(o) == 1 else list(o)
    if args.tile_align is not None:
        opt.setdefault("eval", {})["tile_align"] = args.tile_align


def _dataset(opt, mode, list_root):
    from .dataset import DepthDataset
    d = opt["dataset"]
    kw = {} if list_root is None else {"list_root": list_root}
    if "img_size" in d:
        kw["img_size"] = tuple(d["img_size"])
    for k in ("height_drop", "width_drop"):
        if k in d:
            kw[k] = tuple(d[k])
    for k in ("clip_depth", "drop_edge", "use_right"):
        if k in d:
            kw[k] = d[k]
    return DepthDataset(d["data_path"], d["data_type"], mode, **kw)


def _loader(ds, workers, **kw):
    """collate_raw batches, pinned by the main process; workers only decode files.  They are
    forked while this process has made no HIP call; a process that already has (a caller that
    used the GPU before main()) starts them through a fork server instead."""
    from .dataset import collate_raw
    ctx = None
    if workers:
        ctx = "forkserver" if torch.cuda.is_initialized() else "fork"
    return torch.utils.data.DataLoader(ds, collate_fn=collate_raw, num_workers=workers, pin_memory=True,
                                       persistent_workers=workers > 0, prefetch_factor=4 if workers else None,
                                       multiprocessing_context=ctx, **kw)


def _read_checkpoint(path):
    if not os.path.isfile(path):
        raise SystemExit(f"mdemi.run: checkpoint {path!r} does not exist")
    return torch.load(path, map_location="cpu", weights_only=True)


def main(argv=None) -> int:
    args = _args(argv)
    from .utils.common_utils import dprint, parse, time_log
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    distributed = all(k in os.environ for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"))
    if not distributed:
        rank, world, local_rank = 0, 1, 0

    # 1. the config
    opt = _override(parse(args.opt, write_option=rank == 0 and not args.test), args)
    from .train.builder import (eval_align, eval_boundary, eval_record, eval_tile, grad_match_config, nonfinite_policy,
                                ssi_config)
    from .train.ema import ema_config
    nonfinite_policy(opt)  # a bad train.nonfinite / max_consecutive_skips fails here, before any worker starts
    ema_config(opt)  # and so does a bad train.ema_decay / ema_warmup / ema_validate
    grad_match_config(opt)  # and a bad loss.grad_weight / grad_scales
    ssi_config(opt)  # and a bad loss.ssi_weight / ssi_space / ssi_trim / ssi_norm
    align = eval_align(opt)  # and a bad eval.align
    tile = eval_tile(opt)  # and a bad eval.tile / tile_overlap / tile_align / tile_batch
    boundary = eval_boundary(opt)  # and a bad eval.boundary
    if args.ema and not args.test:
        raise SystemExit("mdemi.run --ema selects the weights --test evaluates; to train with averaged weights set "
                         "train.ema_decay (or --ema-decay)")
    out_dir = opt["output_dir"]
    data_type = opt["dataset"]["data_type"].upper()
    eval_opt = dict(opt.get("eval", {}))

    # 2. the checkpoint, on the CPU
    ck_path = args.checkpoint or (opt.get("checkpoint") or "")
    if args.test and not ck_path:
        raise SystemExit("mdemi.run --test: missing checkpoint -- pass --checkpoint FILE or set the config's "
                         "\"checkpoint\" key")
    ck = _read_checkpoint(ck_path) if ck_path else None
    if args.ema:
        from .predict import require_ema
        require_ema(ck, ck_path, "mdemi.run --test --ema")

    # 3. both loaders and their workers, before the device is selected: no worker is forked
    #    from a process that has made a HIP call (_loader)
    workers = max(0, min(int(opt.get("dataloader", {}).get("num_workers", 0)), MAX_WORKERS))
    from .train.builder import build_model, optimizer_steps_per_epoch
    from .train.loop import EpochStream, TrainBatches, fit
    # the train workers first: starting a pinning loader's iterator initialises HIP in this
    # process (its pin thread selects the device), so the train loader forks while the process
    # is still clean and the test loader, started second, goes through the fork server
    test_ds = _dataset(opt, "test", args.list_root)
    train_it = None
    if not args.test:
        train_ds = _dataset(opt, "train", args.list_root)
        spe = optimizer_steps_per_epoch(opt, world, images=len(train_ds))
        start_epoch = start_step = 0
        if ck is not None and "model_state_dict" in ck:
            # the file's (epoch, iter): optimizer steps completed in that epoch
            start_epoch, start_step = divmod(int(ck.get("epoch") or 0) * spe + int(ck.get("iter") or 0), spe)
        tr = opt.get("train", {})
        stream = EpochStream(len(train_ds), int(opt["dataloader"]["batch_size"]), world, rank, args.seed,
                             int(tr.get("epoch", 1)), int(tr.get("num_accum", 1)), start_epoch, start_step)
        train_loader = _loader(train_ds, workers, batch_sampler=stream)
        train_it = iter(train_loader)
    shard = torch.utils.data.Subset(test_ds, list(range(rank, len(test_ds), world)))
    test_loader = _loader(shard, workers, batch_size=int(eval_opt.get("batch_size", 1)), shuffle=False)
    test_first = [iter(test_loader)]

    # 4. only now the device, the process group, the model
    if not torch.cuda.is_available():
        raise RuntimeError("mdemi.run needs a GPU")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if distributed:
        torch.distributed.init_process_group("nccl", device_id=dev)
    torch.manual_seed(args.seed)
    test_tf = test_ds.transform()

    def test_batches():
        it = test_first.pop() if test_first else iter(test_loader)
        for b in it:
            img, gt, _ = test_tf(b["image"], b["depth"])
            yield img, gt

    from .evaluate import TiledPredictor, evaluate

    def predictor(model):  # eval.tile: the model behind a sliding window
        if tile is None:
            return model
        return TiledPredictor(model, flip_eval=bool(eval_opt.get("flip_eval", False)), **tile)

    try:
        if args.test:
            from .predict import _load_weights
            model = build_model(opt, drop_path=0.0)
            _load_weights(model, ck_path, ema=args.ema)
            model.to(dev).eval()
            metrics = eval_record(evaluate(predictor(model), test_batches(), eval_opt, data_type, weight_by_count=True),
                                  boundary)
            rec = {"type": "test", "checkpoint": ck_path, **metrics}
            if args.ema:
                rec["weights"] = "ema"
            if align != "none":
                rec["align"] = align
            if tile is not None:
                rec.update(tile=list(tile["tile"]), tile_align=tile["align"])
            if rank == 0:
                os.makedirs(out_dir, exist_ok=True)
                with open(os.path.join(out_dir, "log.jsonl"), "a", encoding="utf-8") as f:
                    f.write(json.dumps(rec) + "\n")
            dprint(json.dumps(rec), local_rank=rank)
            return 0

        from .train import build_from_config
        from .train.telemetry import Telemetry
        print_freq = max(1, int(opt.get("train", {}).get("print_freq", 20)))
        telemetry = Telemetry(capacity=max(1024, 2 * print_freq), device=dev)
        trainer = build_from_config(opt, device=dev, world=world, steps_per_epoch=spe, drop_path=args.drop_path,
                                    precision=args.precision, graph=args.graph, telemetry=telemetry)
        best = None
        if ck is not None:
            trainer.resume(ck_path)
            if isinstance(ck.get("best"), (int, float)) and ck.get("best_iter") is not None:
                best = (float(ck["best"]), ck.get("best_epoch"), ck.get("best_iter"))
            dprint(f"resumed {ck_path}: epoch {start_epoch}, step {start_step}", local_rank=rank)
        dprint(time_log(), end="", local_rank=rank)
        batches = TrainBatches(train_it, train_ds.transform(), trainer.num_accum, spe, seed=args.seed, rank=rank,
                               start_epoch=start_epoch, start_step=start_step)

        def validate(model=None):  # fit names the model when it validates averaged weights
            return evaluate(predictor(model if model is not None else trainer.model), test_batches(), eval_opt,
                            data_type, weight_by_count=True)

        return fit(trainer, batches, validate, opt, out_dir, steps_per_epoch=spe, start_epoch=start_epoch,
                   start_step=start_step, max_steps=args.max_steps, rank=rank, world=world, best=best,
                   log=lambda s: dprint(s, local_rank=rank, flush=True))
    finally:
        del train_it
        test_first.clear()
        if distributed and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
