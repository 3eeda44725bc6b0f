"""An exponential moving average of the weights (train.ema_decay): the "shadow" model that
is validated, and from which best.pth is chosen, instead of the raw weights of one step.

ModelEma holds ``module``, a second model of the same configuration whose parameters are the
averages.  Nothing here moves them: FusedAdamW.set_ema hands their addresses to the AdamW
kernel, which updates each average in the sweep that writes its parameter
(mdemi_adamw_step_ema16 / mdemi_adamw_step_dev_ema16) -- inside a captured step too, and not
at all on a step the guarded update drops.  Buffers (BatchNorm running statistics,
num_batches_tracked) are copied from the live model before a validation, not averaged
(DESIGN.md §1c).  Under data parallelism every rank applies the same arithmetic to the same
weights, so the averages agree without a collective.
"""
from __future__ import annotations

import torch

EMA_VALIDATE = ("ema", "both")


def ema_config(opt):
    """(train.ema_decay or None, train.ema_warmup, train.ema_validate), validated."""
    tr = opt.get("train", {})
    decay = tr.get("ema_decay")
    if decay is not None:
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"train.ema_decay must be a number in [0, 1) (or absent / null: off), got {decay!r}")
        decay = float(decay)
    warmup = tr.get("ema_warmup", False)
    if not isinstance(warmup, bool):
        raise ValueError(f"train.ema_warmup must be true or false, got {warmup!r}")
    which = tr.get("ema_validate", "ema")
    if which not in EMA_VALIDATE:
        raise ValueError(f"train.ema_validate must be one of {EMA_VALIDATE}, got {which!r}")
    return decay, warmup, which


class ModelEma:
    """``module``: build_model(opt, drop_path=0.0) loaded from ``model.state_dict()``, in eval
    mode, requires_grad off.  A deepcopy would take along the cached bf16 copies the live
    model's tensors carry (functional.set_b16); a rebuilt model owns every tensor it reads."""

    def __init__(self, opt, model, decay, warmup=False):
        from .builder import build_model
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"ModelEma: decay must be in [0, 1), got {decay!r}")
        self.decay, self.warmup = decay, bool(warmup)
        dev = next(model.parameters()).device
        if dev.type == "meta":
            with torch.device("meta"):
                module = build_model(opt, drop_path=0.0)
        else:
            module = build_model(opt, drop_path=0.0).to(dev)
            module.load_state_dict(model.state_dict())
        module.eval()
        module.requires_grad_(False)
        self.module = module

    def pairs(self, model):
        """{live parameter: its average}, by name, over the parameters an optimizer updates."""
        mine = dict(self.module.named_parameters())
        live = dict(model.named_parameters())
        if mine.keys() != live.keys():
            raise ValueError("ModelEma: the model's parameter names differ from the averaged model's")
        return {p: mine[k] for k, p in live.items() if p.requires_grad}

    @torch.no_grad()
    def sync_buffers(self, model):
        """Copy every buffer of the live model (they are not averaged)."""
        mine = dict(self.module.named_buffers())
        for k, b in model.named_buffers():
            mine[k].copy_(b)

    @torch.no_grad()
    def reset(self, model):
        """Restart the averages from the live weights, in place."""
        self.module.load_state_dict(model.state_dict())

    def state_dict(self):
        return self.module.state_dict()

    def load_state_dict(self, sd):
        """In place: the addresses FusedAdamW's table holds stay valid."""
        self.module.load_state_dict(sd)
