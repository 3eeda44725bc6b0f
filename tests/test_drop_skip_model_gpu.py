"""DropPath skip at the model level: with the skip on (mf.set_drop_skip, the default) a Swin
block and a whole NeW-CRFs train step compute what they compute with it off -- the path
without any mask, which the reference tests pin.  Equalities are exact: a dropped sample's
branch contributes exact zeros either way (DESIGN.md "DropPath skip")."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


class _Skip:
    def __init__(self, mf, on):
        self.mf, self.on, self.prev = mf, on, None

    def __enter__(self):
        self.prev = self.mf.get_drop_skip()
        self.mf.set_drop_skip(self.on)

    def __exit__(self, *a):
        self.mf.set_drop_skip(self.prev)
        return False


def test_switch_default_and_mask_source(mf):
    default = os.environ.get("MDEMI_DROP_SKIP", "1") != "0"  # on unless the environment says 0
    assert mf.get_drop_skip() is default
    s = torch.ones(2, device=DEV)
    with _Skip(mf, True):
        assert mf.drop_live(s) is s and mf.drop_live(None) is None
    with _Skip(mf, False):
        assert mf.drop_live(s) is None
    assert mf.get_drop_skip() is True


def test_swin_block_skip_on_equals_off(mf, monkeypatch):
    """dim 64, 2 heads, shifted windows, B = 4 at 10 x 12 tokens (pads to 14 x 14; 120 rows per
    sample against 128-row tiles), train mode with fixed DropPath scales that hold zeros: whole
    dead tiles, straddling tiles and dead K chunks all occur.  Output, input gradient and every
    parameter gradient are equal with the skip on and off."""
    from mdemi.model.NewCRFs.swin_transformer import SwinTransformerBlock
    B, H, W, C = 4, 10, 12, 64
    keep = 1.0 / 0.7
    scales = [[0.0, 0.0, keep, 0.0], [keep, 0.0, 0.0, 0.0]]  # s1 (attention branch), s2 (MLP branch)
    torch.manual_seed(0)
    blk = SwinTransformerBlock(C, 2, window_size=7, shift_size=3, drop_path=0.3).to(DEV).train()
    blk.H, blk.W = H, W
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(B, H * W, C, device=DEV, generator=g)
    dy = torch.randn(B, H * W, C, device=DEV, generator=g)

    def run(on):
        draws = iter(scales)
        monkeypatch.setattr(mf, "drop_path_scale", lambda batch, p, device: torch.tensor(next(draws), device=device))
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_()
        with _Skip(mf, on):
            y = blk(xi)
            y.backward(dy)
        assert next(draws, None) is None, "the block draws s1 and s2, once each"
        return {"y": y.detach().clone(), "dx": xi.grad.clone(),
                **{n: p.grad.clone() for n, p in blk.named_parameters()}}

    off, on = run(False), run(True)
    assert off.keys() == on.keys() and len(off) > 10
    diff = [k for k in off if not torch.equal(off[k], on[k])]
    assert not diff, diff
    assert all(bool(torch.isfinite(v).all()) for v in on.values())
    # the dropped samples pass through each branch untouched: sample 1 is dead in both
    assert torch.equal(on["y"][1], x[1])


def _opt():
    return {"model": {"name": "newcrfs", "version": "tiny07"}, "eval": {"max_depth_eval": 10.0},
            "optimizer": {"lr": 2e-4, "weight_decay": 0.01, "same_lr": True}, "dataloader": {"batch_size": 4},
            "scheduler": {"pct_start": 0.3}, "train": {"grad_norm": 0.1, "epoch": 1, "num_accum": 1}}


def test_newcrfs_tiny07_three_steps_skip_on_equals_off(mf):
    """NewCRFDepth tiny07, drop_path_rate 0.5, B = 4 at 64 x 96: three Trainer steps from the
    same seed with the skip on and off give equal losses and equal parameters (the draws are
    the same calls in the same order, so both runs drop the same samples)."""
    from mdemi.train import build_from_config
    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(4, 3, 64, 96, generator=g).to(DEV), (torch.rand(4, 1, 64, 96, generator=g) * 9 + 0.5).to(DEV))
            for _ in range(3)]

    def run(on):
        with _Skip(mf, on):
            torch.manual_seed(0)
            t = build_from_config(_opt(), device=DEV, steps_per_epoch=10, drop_path=0.5)
            torch.manual_seed(1)
            losses = [t.step([b]).detach().clone() for b in data]
            torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in t.model.state_dict().items()}

    loss_off, sd_off = run(False)
    loss_on, sd_on = run(True)
    assert all(bool(torch.isfinite(v).all()) for v in loss_on)
    assert [v.item() for v in loss_on] == [v.item() for v in loss_off]
    diff = [k for k in sd_off if not torch.equal(sd_off[k], sd_on[k])]
    assert not diff, diff
