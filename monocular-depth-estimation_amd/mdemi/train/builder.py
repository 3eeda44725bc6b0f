"""Config-driven train step: the restated run.py's construction phase.

The reference snapshot has no run.py (evidence
output/test/wandb/latest-run/files/wandb-metadata.json:16 and the traceback
in run-1pklfwui.wandb), but its JSON configs (json/{nyu,kitti,online}/**)
name every choice the train step makes.  ``build_from_config(opt)`` maps an
``opt`` as returned by ``utils.common_utils.parse`` (common_utils.py:34-52),
unchanged, onto this framework's objects:

  model.name            adabins        -> UnetAdaptiveBins.build(num_bins, min, max)   unet_adaptive_bins.py:126-139
                        newcrfs        -> NewCRFDepth('large07', max_depth=max)        NewCRFDepth.py:15
                        depthformer_v8 -> DepthformerV8.build(opt.model, min, max)      depthformer_v8.py:84-102
                        oda2_red_order_swin2 -> ODA2OrderedSwin2RegModel.build(...)    oda2_red_order_swin2.py:98-118
                           (model.use_checkpoint, default the reference's True, toggles the
                           encoder's activation checkpointing)
  model.bn_momentum     -> every BatchNorm's momentum
  loss.alpha/beta/per_image -> SILogLoss (+ loss.chamfer_weight x BinsChamferLoss on the bins;
                        ODA2: loss.si_weight x the mean SILog over every output the model returns
                        -- the head's earlier outputs get gradient from nowhere else, its
                        depth indices are detached, :246-253)
  loss.grad_weight      -> absent / 0: off.  A finite float > 0: + grad_weight x GradMatchLoss, the
                           multi-scale gradient-matching term on the same (resized) depth, per image
                           or per batch as loss.per_image says; ODA2: averaged over every output
                           like si_weight x SILog.  loss.grad_scales: its scales, 1..4 (default 4).
                           This framework's own keys and definition (a decision)
  loss.ssi_weight       -> absent / 0: off.  A finite float > 0: + ssi_weight x SSILoss, the scale- and
                           shift-invariant data term on the same (resized) depth, reduced as
                           loss.per_image says; ODA2: averaged over every output.  loss.ssi_space
                           "depth" (default) | "disp", loss.ssi_trim in [0, 0.5] (default 0),
                           loss.ssi_norm "none" (default) | "gt_var".  While it is on, loss.si_weight
                           also weighs SILog on the single-output models, and si_weight 0 launches
                           no SILog.  This framework's own keys and definition
  optimizer.lr/weight_decay/betas/eps/same_lr -> FusedAdamW; with get_1x_lr_params
                        (unet_adaptive_bins.py:111-117) and same_lr false: two groups,
                        encoder at lr/10, the rest at lr
  scheduler.name=onecycle, pct_start/div_factor/final_div_factor/cycle_momentum
                        -> OneCycleLR (max_lr = each group's lr; total = epoch x
                           optimizer steps per epoch)
  train.grad_norm       -> global-norm clip folded into the AdamW step
  train.nonfinite       -> "stop" (default): a non-finite step ends the run; "skip": the guarded
                           AdamW step drops it on the device and the run goes on, until more
                           than train.max_consecutive_skips (default 10) follow one another
                           (a decision; the reference does not pin it)
  train.ema_decay       -> absent / null: off.  A float in [0, 1): ModelEma (train.ema), an averaged
                           copy of the weights the AdamW kernel updates in its own sweep; it is
                           what gets validated and what best.pth is chosen on.  train.ema_warmup
                           (bool) ramps the decay as min(decay, (1 + n) / (10 + n));
                           train.ema_validate "ema" (default) or "both" (the raw weights too)
  train.num_accum       -> micro-steps accumulated per optimizer step (DDP no_sync
                           on all but the last)
  train.freeze_encoder_bn / freeze_all_bn -> BatchNorm modules kept in eval mode
                           (common_utils.py:78-81 freeze_bn)
  eval.min/max_depth_eval -> the model's depth range (NYU 10 m, KITTI 80 m)

What is a decision rather than parity (the reference does not pin it) is
listed in DESIGN.md §1 (restated train step).  The depth range follows
upstream AdaBins / NeW-CRFs (min 1e-3, max = the dataset's max_depth_eval)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .loss import BinsChamferLoss, GradMatchLoss, SILogLoss, SSILoss, resize_to_gt
from .optim import FusedAdamW, OneCycleLR

MODEL_NAMES = ("adabins", "newcrfs", "depthformer_v8", "oda2_red_order_swin2")
# training-split sizes behind the default steps-per-epoch: depth_dataset.py:79 reads
# train_test_inputs/NYU/nyu_train_36k.txt (36,253 pairs), :49 KITTI/kitti_eigen_train.txt
# (23,158); ONLINE's kitti_benchmark_train.txt is a missing blob, so KITTI's count stands in
TRAIN_IMAGES = {"NYU": 36253, "KITTI": 23158, "ONLINE": 23158}


def _depth_range(opt):
    ev = opt.get("eval", {})
    return float(ev.get("min_depth_eval", 1e-3)), float(ev.get("max_depth_eval", 10.0))


def build_model(opt, drop_path=None):
    m = opt["model"]
    name = m["name"]
    dmin, dmax = _depth_range(opt)
    if name == "adabins":
        from ..model.Adabins import UnetAdaptiveBins
        model = UnetAdaptiveBins.build(int(m.get("num_bins", 256)), dmin, dmax)
    elif name == "newcrfs":
        from ..model.NewCRFs import NewCRFDepth
        kw = {} if drop_path is None else {"drop_path_rate": drop_path}
        model = NewCRFDepth(version=m.get("version", "large07"), inv_depth=False, max_depth=dmax, **kw)
    elif name == "depthformer_v8":
        from ..model.Depthformer import DepthformerV8
        model = DepthformerV8.build(m, dmin, dmax)
    elif name == "oda2_red_order_swin2":
        from ..model.ODA2 import ODA2OrderedSwin2RegModel
        kw = {"use_checkpoint": bool(m.get("use_checkpoint", True))}
        if drop_path is not None:
            kw["path_drop_prob"] = drop_path
        model = ODA2OrderedSwin2RegModel.build(m, dmin, dmax, **kw)
    else:
        raise ValueError(f"model.name {name!r} is not on this framework's path (one of {MODEL_NAMES})")
    if "bn_momentum" in m:
        for mod in model.modules():
            if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                mod.momentum = float(m["bn_momentum"])
    return model


# loss.* keys of the in-scope reference configs; sog_weight names a loss term this framework
# does not implement (0.0 in every in-scope config) and reduction_ratio configures only that
# term -- a nonzero sog_weight is refused rather than silently dropped
# grad_weight / grad_scales (the gradient-matching term) and ssi_weight / ssi_space / ssi_trim / ssi_norm
# (the scale- and shift-invariant term) are this framework's own keys
LOSS_KEYS = ("alpha", "beta", "per_image", "chamfer_weight", "si_weight", "sog_weight", "reduction_ratio",
             "grad_weight", "grad_scales", "ssi_weight", "ssi_space", "ssi_trim", "ssi_norm")


def grad_match_config(opt):
    """(loss.grad_weight, loss.grad_scales), validated: a finite weight >= 0 (absent: 0.0, the
    term is off) and an integer number of scales 1..4 (default 4)."""
    lo = opt.get("loss", {})
    w = lo.get("grad_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < 0:
        raise ValueError(f"loss.grad_weight must be a finite number >= 0, got {w!r}")
    from ..functional import check_grad_scales
    return float(w), check_grad_scales(lo.get("grad_scales", 4), "loss.grad_scales")


def ssi_config(opt):
    """(loss.ssi_weight, loss.ssi_space, loss.ssi_trim, loss.ssi_norm), validated: a finite weight
    >= 0 (absent: 0.0, the term is off), "depth" (default) or "disp", a finite trim in [0, 0.5]
    (default 0.0) and "none" (default) or "gt_var"."""
    lo = opt.get("loss", {})
    w = lo.get("ssi_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < 0:
        raise ValueError(f"loss.ssi_weight must be a finite number >= 0, got {w!r}")
    from ..functional import check_ssi_options
    return (float(w),) + check_ssi_options(lo.get("ssi_space", "depth"), lo.get("ssi_trim", 0.0),
                                           lo.get("ssi_norm", "none"),
                                           ("loss.ssi_space", "loss.ssi_trim", "loss.ssi_norm"))


class TrainLoss:
    """SILog on the depth (+ chamfer_weight x the bin chamfer loss on AdaBins' edges /
    Depthformer's centres when loss.chamfer_weight > 0, + grad_weight x the multi-scale
    gradient-matching loss on the same depth when loss.grad_weight > 0, + ssi_weight x the
    scale- and shift-invariant loss on the same depth when loss.ssi_weight > 0; with that term
    on, si_weight weighs SILog on every model and si_weight 0 leaves SILog out)."""

    def __init__(self, opt, model_name):
        lo = opt.get("loss", {})
        unknown = sorted(set(lo) - set(LOSS_KEYS))
        if unknown:
            raise ValueError(f"loss keys {unknown} are not implemented by this framework (known: {LOSS_KEYS})")
        if float(lo.get("sog_weight", 0.0)) != 0.0:
            raise ValueError(f"loss.sog_weight={lo['sog_weight']}: the SOG loss term is not implemented "
                             "(every in-scope reference config sets it to 0.0)")
        self.grad_weight, grad_scales = grad_match_config(opt)
        self.ssi_weight, ssi_space, ssi_trim, ssi_norm = ssi_config(opt)
        dmin, _ = _depth_range(opt)
        self.silog = SILogLoss(alpha=float(lo.get("alpha", 10.0)), beta=float(lo.get("beta", 0.15)),
                               per_image=bool(lo.get("per_image", False)), min_depth=dmin)
        self.w = float(lo.get("chamfer_weight", 0.0))
        self.chamfer = BinsChamferLoss(dmin, from_edges=(model_name == "adabins")) if self.w > 0 else None
        # weight 0 (or no key): no module, nothing of the term is launched
        self.grad = GradMatchLoss(grad_scales, per_image=self.silog.per_image, min_depth=dmin) \
            if self.grad_weight > 0 else None
        self.ssi = SSILoss(ssi_space, ssi_trim, ssi_norm, per_image=self.silog.per_image, min_depth=dmin) \
            if self.ssi_weight > 0 else None
        self.multi = model_name == "oda2_red_order_swin2"
        self.si_weight = float(lo.get("si_weight", 1.0))

    def __call__(self, out, gt):
        if self.multi:  # (out, outs, attn): every output, each upsampled to the GT
            outs = [resize_to_gt(o, gt) for o in out[1]]

            def mean_of(term, weight):
                total = term(outs[0], gt)
                for o in outs[1:]:
                    total = total + term(o, gt)
                return total * (weight / len(outs))

            loss = None if self.ssi is not None and self.si_weight == 0 else mean_of(self.silog, self.si_weight)
            if self.grad is not None:
                gm = mean_of(self.grad, self.grad_weight)
                loss = gm if loss is None else loss + gm
            if self.ssi is not None:
                ssi = mean_of(self.ssi, self.ssi_weight)
                loss = ssi if loss is None else loss + ssi
            return loss
        pred = out[0] if isinstance(out, tuple) else out
        pred = resize_to_gt(pred, gt)  # a half-resolution prediction, once for every term
        if self.ssi is None:  # si_weight is not read on this path while the SSI term is off
            loss = self.silog(pred, gt)
        elif self.si_weight == 0:
            loss = None
        else:
            loss = self.silog(pred, gt) if self.si_weight == 1 else self.si_weight * self.silog(pred, gt)
        if self.grad is not None:
            gm = self.grad_weight * self.grad(pred, gt)
            loss = gm if loss is None else loss + gm
        if self.ssi is not None:
            ssi = self.ssi_weight * self.ssi(pred, gt)
            loss = ssi if loss is None else loss + ssi
        if self.chamfer is not None:
            loss = loss + self.w * self.chamfer(out[1], gt)
        return loss


def param_groups(model, opt):
    o = opt.get("optimizer", {})
    lr = float(o["lr"])
    same_lr = bool(o.get("same_lr", False))
    if not same_lr and hasattr(model, "get_1x_lr_params"):
        return [{"params": list(model.get_1x_lr_params()), "lr": lr / 10.0},
                {"params": list(model.get_10x_lr_params()), "lr": lr}]
    return [{"params": list(model.parameters()), "lr": lr}]


NONFINITE_POLICIES = ("stop", "skip")


def nonfinite_policy(opt):
    """(train.nonfinite, train.max_consecutive_skips), validated."""
    tr = opt.get("train", {})
    policy = tr.get("nonfinite", "stop")
    if policy not in NONFINITE_POLICIES:
        raise ValueError(f"train.nonfinite must be one of {NONFINITE_POLICIES}, got {policy!r}")
    limit = tr.get("max_consecutive_skips", 10)
    if isinstance(limit, bool) or not isinstance(limit, int) or limit < 0:
        raise ValueError(f"train.max_consecutive_skips must be a non-negative integer, got {limit!r}")
    return policy, limit


def eval_align(opt):
    """eval.align, validated: "none" (also when the key is absent), "median", "lstsq" or
    "lstsq_disp" -- the per-image alignment the evaluator applies before the metrics."""
    from ..utils.depth_utils import check_align_mode
    return check_align_mode(opt.get("eval", {}).get("align", "none"))


def eval_boundary(opt):
    """eval.boundary, validated: None when the key is absent or false; true -> the defaults
    (1.05, 1.25, 10); {"t_min": .., "t_max": .., "n": ..} -> (t_min, t_max, n), the range and
    number of depth-ratio thresholds of the boundary F1 the evaluator reports next to the nine
    metrics.  Unknown keys, t_min <= 1, t_max < t_min, n outside 1..16 and
    booleans as numbers raise a ValueError that names the key."""
    from ..utils.depth_utils import check_boundary
    return check_boundary(opt.get("eval", {}).get("boundary"))


def eval_record(metrics, boundary):
    """evaluate()'s result as the fields of a "valid" / "test" record: floats, boundary_images an
    integer, and under eval.boundary "boundary": [t_min, t_max, n]."""
    rec = {k: float(v) for k, v in metrics.items()}
    if boundary is not None:
        rec["boundary_images"] = int(rec.get("boundary_images", 0))
        rec["boundary"] = list(boundary)
    return rec


TILE_KEYS = ("tile", "tile_overlap", "tile_align", "tile_batch")


def eval_tile(opt):
    """eval.tile / tile_overlap / tile_align / tile_batch, validated: None when eval.tile is absent
    (the other three must then be absent too), else the TiledPredictor arguments {"tile": (h, w),
    "overlap": (oy, ox) (default: a quarter of the tile), "align": "none" | "lstsq" | "lstsq_disp",
    "tile_batch": n | None, "max_depth": eval.max_depth_eval}."""
    from ..utils.depth_utils import _pair, check_tile_align
    ev = opt.get("eval", {})
    if ev.get("tile") is None:
        extra = [k for k in TILE_KEYS[1:] if k in ev]
        if extra:
            raise ValueError(f"eval.{extra[0]} is set but eval.tile is not: tiled inference needs eval.tile: [h, w]")
        return None
    tile = ev["tile"]
    if not isinstance(tile, (list, tuple)):
        raise ValueError(f"eval.tile must be a list [h, w] of two positive integers, got {tile!r}")
    th, tw = _pair(tile, "eval.tile", 1)
    oy, ox = _pair(ev["tile_overlap"], "eval.tile_overlap", 0) if "tile_overlap" in ev else (th // 4, tw // 4)
    if oy >= th or ox >= tw:
        raise ValueError(f"eval.tile_overlap {[oy, ox]} must be smaller than eval.tile {[th, tw]}")
    align = check_tile_align(ev.get("tile_align", "none"))
    batch = ev.get("tile_batch")
    if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or batch < 1):
        raise ValueError(f"eval.tile_batch must be a positive integer, got {batch!r}")
    max_depth = ev.get("max_depth_eval")
    if align == "lstsq_disp" and not (isinstance(max_depth, (int, float)) and max_depth > 0):
        raise ValueError(f"eval.tile_align 'lstsq_disp' needs eval.max_depth_eval > 0, got {max_depth!r}")
    return {"tile": (th, tw), "overlap": (oy, ox), "align": align, "tile_batch": batch, "max_depth": max_depth}


def build_optimizer(model, opt, capturable=False):
    o = opt.get("optimizer", {})
    betas = tuple(float(b) for b in o.get("betas", (0.9, 0.999)))
    kw = {"skip_nonfinite": True} if nonfinite_policy(opt)[0] == "skip" else {}
    return FusedAdamW(param_groups(model, opt), lr=float(o["lr"]), betas=betas, eps=float(o.get("eps", 1e-8)),
                      weight_decay=float(o.get("weight_decay", 0.0)),
                      max_grad_norm=float(opt.get("train", {}).get("grad_norm", 0.0)), capturable=capturable, **kw)


def optimizer_steps_per_epoch(opt, world=1, images=None):
    data_type = opt.get("dataset", {}).get("data_type", "NYU")
    images = images if images is not None else TRAIN_IMAGES.get(data_type, 36253)
    batch = int(opt.get("dataloader", {}).get("batch_size", 8))
    loader_len = math.ceil(images / (batch * world))
    return max(1, loader_len // int(opt.get("train", {}).get("num_accum", 1)))


def build_scheduler(optimizer, opt, steps_per_epoch):
    s = opt.get("scheduler", {})
    name = s.get("name", "onecycle")
    if name != "onecycle":
        raise ValueError(f"scheduler.name {name!r}: only 'onecycle' is configured by the reference")
    total = int(opt.get("train", {}).get("epoch", 1)) * int(steps_per_epoch)
    return OneCycleLR(optimizer, max_lr=[g["lr"] for g in optimizer.param_groups], total_steps=total,
                      pct_start=float(s.get("pct_start", 0.3)), div_factor=float(s.get("div_factor", 25.0)),
                      final_div_factor=float(s.get("final_div_factor", 1e4)),
                      cycle_momentum=bool(s.get("cycle_momentum", True)))


def freeze_bn(model):
    """common_utils.py:78-81."""
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.eval()


def quiesce_process_group(works=(), groups=()):
    """Before a hipGraph capture on a process whose RCCL process groups have run eager
    collectives: wait for each eager Work, then block until every ProcessGroupNCCL's
    watchdog thread has retired every one of them (ProcessGroupNCCL::waitForPendingWorks
    returns once the watchdog's work list and its completed-work list are both empty).
    The watchdog polls each listed work's HIP event (hipEventQuery); such a query issued
    while this thread holds a global-mode capture is a capture-unsafe call from another
    thread, which invalidates the capture and aborts the process.  Collectives issued
    during the capture are never listed, so once the lists are empty nothing else can
    query mid-capture.  ``groups``: the process groups the captured step issues
    collectives on besides the default one (GradAllReduce(group=...)); each "nccl" group
    is drained.  A no-op without an initialised process group; gloo groups have no
    watchdog (nothing to wait for).  The drain is a private ProcessGroupNCCL method
    (torch 2.10: ``_wait_for_pending_works``); if a torch update removes it this raises
    rather than capture without the guarantee."""
    import torch.distributed as dist
    for w in works:
        w.wait()
    torch.cuda.synchronize()
    if not (dist.is_available() and dist.is_initialized()):
        return
    todo = [dist.distributed_c10d._get_default_group()]
    for g in groups:
        if g is not None and all(g is not t for t in todo):
            todo.append(g)
    for pg in todo:
        if dist.get_backend(pg) != "nccl":
            continue
        drain = getattr(pg, "_wait_for_pending_works", None)
        if drain is None:
            raise RuntimeError(
                f"quiesce_process_group: torch {torch.__version__}'s ProcessGroupNCCL has no "
                "_wait_for_pending_works(); a global-mode hipGraph capture could race the RCCL "
                "watchdog's event queries -- capture refused (run the step eagerly: graph=False)")
        drain()


class Trainer:
    """One optimizer step = num_accum micro-batches of forward + loss/num_accum + backward
    (gradients accumulate in place), then the gradient all-reduce (DDP), the clipped
    AdamW update and one OneCycle step.

    precision "bf16": every libmdemi GEMM (Linear, conv, attention products; forward and
    backward) runs with bf16 operands and fp32 accumulation -- torch.autocast's matmul
    numerics -- while master weights, optimizer state and the other kernels stay fp32.

    graph=True: the first two calls run eagerly (they settle GEMM autotuning, every
    workspace, the optimizer state and, data-parallel, the RCCL communicator), the third
    captures the whole step -- forward, loss, backward, the bucketed RCCL all-reduces the
    backward hooks launch, clip and AdamW (1/world folded in) with its schedule read on the
    device -- into a hipGraph (torch.cuda.CUDAGraph) and replays it.  Gradients are
    persistent either way: DDP bucket views, or (single process) the tensors the captured
    backward hands to each parameter, which every replay rewrites; every later call copies its batch into the static input buffers and
    replays.  Data-parallel, the hooks run once, at capture: the bucket launch order is
    recorded then and every replay issues the same collective sequence on every rank.
    Each call is exactly one optimizer step.  Dropout seeds are drawn on the GPU, so
    masks differ per replay."""

    def __init__(self, opt, model, criterion, optimizer, scheduler, ddp=None, precision="fp32", graph=False,
                 telemetry=None, ema=None):
        tr = opt.get("train", {})
        self.opt, self.model, self.criterion = opt, model, criterion
        # train.ema.ModelEma (or None): the averaged weights; the optimizer already holds their
        # addresses (FusedAdamW.set_ema), the trainer saves, restores and hands them to fit
        self.ema = ema
        # train.telemetry.Telemetry (or None): one record per optimizer step, pushed on the
        # step's stream right after the update -- inside the capture in graph mode
        self.telemetry = telemetry
        self.optimizer, self.scheduler, self.ddp = optimizer, scheduler, ddp
        self.num_accum = int(tr.get("num_accum", 1))
        self.freeze_encoder_bn = bool(tr.get("freeze_encoder_bn", False))
        self.freeze_all_bn = int(tr.get("freeze_all_bn", -1))
        self.epoch = 0
        from .. import functional as mf
        if precision not in mf.PRECISIONS:
            raise ValueError(f"precision must be one of {mf.PRECISIONS}, got {precision!r}")
        self.precision = precision
        self.graph = bool(graph)
        if self.graph:
            if not getattr(optimizer, "capturable", False):
                raise ValueError("graph=True needs FusedAdamW(capturable=True)")
            if scheduler is not None:
                optimizer.set_schedule(scheduler.hyper_table())
        self._graph = None
        self._graph_layout = None
        self._eager_calls = 0
        if ddp is not None and ddp.world > 1 and hasattr(optimizer, "grad_scale"):
            # the all-reduce leaves gradient sums; the AdamW step takes them at 1/world (its
            # clip norm too), bit for bit what scaling the buckets first would give
            ddp.scale_in_finish = False
            optimizer.grad_scale = 1.0 / ddp.world

    def train_mode(self):
        self.model.train()
        enc = getattr(self.model, "encoder", None)
        if self.freeze_encoder_bn and enc is not None:
            freeze_bn(enc)
        if 0 <= self.freeze_all_bn <= self.epoch:
            freeze_bn(self.model)

    def step(self, batches):
        """batches: num_accum (image, gt) pairs; returns the summed (scaled) loss tensor."""
        if len(batches) != self.num_accum:
            raise ValueError(f"Trainer.step: expected {self.num_accum} micro-batches (train.num_accum), "
                             f"got {len(batches)}")
        from .. import functional as mf
        if self.graph:
            return self._graph_step(batches)
        with mf.matmul_precision(self.precision):
            return self._eager_step(batches)

    def _graph_step(self, batches):
        from .. import functional as mf
        if self._graph is not None and self.optimizer.layout_version != self._graph_layout:
            # optimizer state was replaced (load_state_dict with new tensors): the captured
            # pointer table is stale -- rebuild it with one eager step, then re-capture.
            # Each replay leaves its gradients in place (the captured backward writes them,
            # nothing zeroes them), so they are dropped first: the eager step's backward
            # must not accumulate onto the last replay's gradients
            self._graph = None
            self._eager_calls = 1
            self._zero_grad()
        if self._graph is None:
            if self._eager_calls < 2:  # warm-up: autotuning, workspaces, optimizer state, communicator
                self._eager_calls += 1
                with mf.matmul_precision(self.precision):
                    return self._eager_step(batches)
            self._static = [(img.clone(), gt.clone()) for img, gt in batches]
            # without DDP buckets the gradients are None here: the captured backward hands
            # each parameter the tensor its gradient kernel writes (AccumulateGrad steals it,
            # from the graph's pool), so a replay rewrites .grad in place -- no per-parameter
            # zero fill and accumulate-add in the graph (~1400 launches per Depthformer step)
            self._zero_grad()
            if self.ddp is not None:
                # no eager collective may still be listed with the process group's watchdog
                # when the global-mode capture begins (quiesce_process_group)
                quiesce_process_group(groups=(self.ddp.group,))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), mf.matmul_precision(self.precision):
                self._static_loss = self._body(self._static)
                if self.ddp is not None:
                    self.ddp.zero_grad()  # bucket views keep their (captured) addresses
            self._graph = g
            self._graph_layout = self.optimizer.layout_version
        else:
            for (si, sg), (img, gt) in zip(self._static, batches):
                si.copy_(img, non_blocking=True)
                sg.copy_(gt, non_blocking=True)
        self._graph.replay()
        self.optimizer.replayed()  # host mirrors of the device step counters
        if self.scheduler is not None:
            self.scheduler.step()
        return self._static_loss

    def _body(self, batches):
        """Micro-batches (all but the last under no_sync), the gradient exchange and the
        optimizer update: no host synchronisation and no host-side hyperparameter in the
        capturable case, so the same code is what a hipGraph records."""
        total = None
        for i, (img, gt) in enumerate(batches):
            last = i == len(batches) - 1
            ctx = self.ddp.no_sync() if (self.ddp is not None and not last) else _null()
            with ctx:
                loss = self.criterion(self.model(img), gt)
                if self.num_accum > 1:
                    loss = loss * (1.0 / self.num_accum)
                loss.backward()
            total = loss.detach() if total is None else total + loss.detach()
        if self.ddp is not None:
            self.ddp.finish()
        self.optimizer.step()
        if self.telemetry is not None:
            self.telemetry.push(total, self.optimizer)
        return total

    def save(self, prefix, save_dir, current_iter, best_value, best_epoch=None, best_iter=None, model_only=False):
        """common_utils.save_checkpoint of this trainer's model and optimizer at self.epoch."""
        from ..utils.common_utils import save_checkpoint
        extra = None
        if self.ema is not None:  # two more keys; the reference's loaders ignore them
            extra = {"ema_state_dict": self.ema.state_dict(),
                     "ema_meta": {"decay": self.ema.decay, "warmup": self.ema.warmup,
                                  "updates": self.optimizer.ema_updates()}}
        save_checkpoint(prefix, self.model, self.optimizer, self.epoch, current_iter, best_value, save_dir,
                        best_epoch=best_epoch, best_iter=best_iter, model_only=model_only, extra=extra)

    def buffers_finite(self):
        """Whether every floating-point buffer of the model (BatchNorm running statistics) is
        finite: one torch.isfinite per buffer and one host read.  The guarded optimizer step
        cannot protect them -- a forward that overflowed has already written its batch
        statistics -- so the driver asks before a checkpoint under train.nonfinite "skip"."""
        bad = [~torch.isfinite(b).all() for b in self.model.buffers() if torch.is_floating_point(b)]
        return not bad or not bool(torch.stack(bad).any().item())

    def resume(self, path):
        """Load a save_checkpoint file (the reference's format): model weights, optimizer
        state (moments and per-parameter step counts), epoch, and the OneCycle position
        = optimizer steps taken.  A captured step is re-captured after the next eager step
        when the load replaced state tensors (FusedAdamW.layout_version).  With averaged
        weights (self.ema) the file's ema_state_dict and update count are restored in place;
        a file without them restarts the averages from the loaded weights.  Returns the file's
        dict."""
        from ..utils.common_utils import load_checkpoint
        dev = next(self.model.parameters()).device
        ck = load_checkpoint(path, self.model, self.optimizer, map_location=dev)
        if self.ema is not None:
            if ck.get("ema_state_dict") is not None:
                self.ema.load_state_dict(ck["ema_state_dict"])
                self.optimizer.set_ema_updates(int((ck.get("ema_meta") or {}).get("updates", 0)))
            else:
                self.ema.reset(self.model)
                self.optimizer.set_ema_updates(0)
                from ..utils.common_utils import dprint
                dprint(f"{path} holds no ema_state_dict: the averaged weights start from the loaded weights")
        self.epoch = int(ck.get("epoch", 0) or 0)
        if self.scheduler is not None:
            self.scheduler.set_position(self.optimizer.step_count)
        self.train_mode()
        return ck

    def _zero_grad(self):
        if self.ddp is not None:
            self.ddp.zero_grad()  # bucket views stay in place
        else:
            self.optimizer.zero_grad(set_to_none=True)

    def _eager_step(self, batches):
        total = self._body(batches)
        if self.scheduler is not None:
            self.scheduler.step()
        self._zero_grad()
        return total


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def build_from_config(opt, device=None, world=1, steps_per_epoch=None, ddp_bucket_mb=64.0, drop_path=None,
                      precision=None, graph=False, ddp=None, telemetry=None):
    """opt (parse()'s dict) -> Trainer.  device='meta' builds every object without
    allocating parameters (config validation); world > 1 (or ddp=True, e.g. a world-1
    RCCL group) wraps the gradients in the bucketed RCCL all-reduce (needs an
    initialised process group).  precision (default: train.precision or "fp32") and
    graph select the mixed-precision / hipGraph-captured step (Trainer); telemetry
    (train.telemetry.Telemetry) records every step's loss and gradient norm on the device."""
    name = opt["model"]["name"]
    from .ema import ModelEma, ema_config
    ema_decay, ema_warmup, _ = ema_config(opt)  # a bad train.ema_* key fails before anything is built
    if device is not None and torch.device(device).type == "meta":
        with torch.device("meta"):
            model = build_model(opt, drop_path)
    else:
        model = build_model(opt, drop_path)
        if device is not None:
            model = model.to(device)
    criterion = TrainLoss(opt, name)
    optimizer = build_optimizer(model, opt, capturable=graph)
    spe = steps_per_epoch if steps_per_epoch is not None else optimizer_steps_per_epoch(opt, world)
    scheduler = build_scheduler(optimizer, opt, spe)
    grad_ar = None
    if (world > 1) if ddp is None else ddp:
        from .ddp import GradAllReduce, broadcast_parameters
        broadcast_parameters(model)
        grad_ar = GradAllReduce(model, bucket_mb=ddp_bucket_mb)
    ema = None
    if ema_decay is not None:  # after the broadcast: every rank's average starts from rank 0's weights
        ema = ModelEma(opt, model, ema_decay, ema_warmup)
        optimizer.set_ema(ema.pairs(model), ema_decay, ema_warmup)
    precision = precision or opt.get("train", {}).get("precision", "fp32")
    trainer = Trainer(opt, model, criterion, optimizer, scheduler, grad_ar, precision=precision, graph=graph,
                      telemetry=telemetry, ema=ema)
    trainer.train_mode()
    return trainer
