"""Paired GEMM launches at the model level: with pairing on a Swin block and a NeW-CRFs train
step compute, bit for bit, what they compute with pairing off -- eagerly and as a captured
graph; under the tuner's default and with each one-launch arm forced, where the test also
requires that calls really took that arm (mdemi_gemm_pair_last_arm after every call)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARMS = pytest.mark.parametrize("arm", [-1, 1, 2], ids=["tuned", "pair_v11", "pair_v8"])


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


class _Pair:
    """Pairing on / off with a forced arm for the block; self.arms: the arm every call of the
    library's paired entry ran."""

    def __init__(self, on, arm=-1):
        from mdemi import _lib as L
        self.L, self.lib, self.on, self.arm, self.arms = L, L.load(), on, arm, []

    def __enter__(self):
        self.L.check(self.lib.mdemi_gemm_pair_set_options(int(self.on), self.arm), "pair_set_options")
        self.entry = self.lib.mdemi_gemm_f32_pair

        def recorded(*a):
            rc = self.entry(*a)
            self.arms.append(self.lib.mdemi_gemm_pair_last_arm())
            return rc

        self.lib.mdemi_gemm_f32_pair = recorded
        return self

    def __exit__(self, *a):
        self.lib.mdemi_gemm_f32_pair = self.entry
        self.lib.mdemi_gemm_pair_set_options(1, -1)
        return False


def _check_arms(off, on, arm):
    assert off.arms == [], "pairing off: the paired entry is not entered"
    assert on.arms, "pairing on: no call reached the paired entry"
    if arm > 0:  # the forced arm ran wherever the pair was eligible, and it was somewhere
        assert set(on.arms) <= {0, arm} and on.arms.count(arm) > 0, on.arms


@ARMS
@pytest.mark.parametrize("skip", [True, False], ids=["drop_skip_on", "drop_skip_off"])
def test_swin_block_pair_on_equals_off(mf, monkeypatch, skip, arm):
    """dim 96, 3 heads, batch 4 at 14 x 14 tokens, drop_path 0.2 with fixed draws that drop a
    sample in each branch: output, dx and every parameter gradient are equal."""
    from mdemi.model.NewCRFs.swin_transformer import SwinTransformerBlock
    B, H, W, C = 4, 14, 14, 96
    keep = 1.0 / 0.8
    scales = [[keep, 0.0, keep, keep], [keep, keep, 0.0, keep]]
    torch.manual_seed(0)
    blk = SwinTransformerBlock(C, 3, window_size=7, shift_size=3, drop_path=0.2).to(DEV).train()
    blk.H, blk.W = H, W
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(B, H * W, C, device=DEV, generator=g)
    dy = torch.randn(B, H * W, C, device=DEV, generator=g)
    prev = mf.get_drop_skip()
    mf.set_drop_skip(skip)

    def run(pair):
        draws = iter(scales)
        monkeypatch.setattr(mf, "drop_path_scale", lambda batch, p, device: torch.tensor(next(draws), device=device))
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_()
        with pair:
            y = blk(xi)
            y.backward(dy)
        return {"y": y.detach().clone(), "dx": xi.grad.clone(),
                **{n: p.grad.clone() for n, p in blk.named_parameters()}}

    p_off, p_on = _Pair(False), _Pair(True, arm)
    try:
        off, on = run(p_off), run(p_on)
    finally:
        mf.set_drop_skip(prev)
    assert off.keys() == on.keys() and len(off) > 10
    diff = [k for k in off if not torch.equal(off[k], on[k])]
    assert not diff, diff
    assert all(bool(torch.isfinite(v).all()) for v in on.values())
    _check_arms(p_off, p_on, arm)


def _opt():
    return {"model": {"name": "newcrfs", "version": "tiny07"}, "eval": {"max_depth_eval": 10.0},
            "optimizer": {"lr": 2e-4, "weight_decay": 0.01, "same_lr": True}, "dataloader": {"batch_size": 4},
            "scheduler": {"pct_start": 0.3}, "train": {"grad_norm": 0.1, "epoch": 1, "num_accum": 1}}


@ARMS
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_newcrfs_tiny07_two_steps_pair_on_equals_off(mf, graph, arm):
    """NewCRFDepth tiny07, drop_path_rate 0.2, B = 4 at 64 x 96: two Trainer steps from the same
    seed with pairing on and off give equal losses and equal weights; the captured step too
    (whatever the pair tuner has or has not cached when the capture begins)."""
    from mdemi.train import build_from_config
    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(4, 3, 64, 96, generator=g).to(DEV), (torch.rand(4, 1, 64, 96, generator=g) * 9 + 0.5).to(DEV))
            for _ in range(2)]

    def run(pair):
        with pair:
            torch.manual_seed(0)
            t = build_from_config(_opt(), device=DEV, steps_per_epoch=10, drop_path=0.2, graph=graph)
            torch.manual_seed(1)
            losses = [t.step([b]).detach().clone() for b in data]
            torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in t.model.state_dict().items()}

    p_off, p_on = _Pair(False), _Pair(True, arm)
    loss_off, sd_off = run(p_off)
    loss_on, sd_on = run(p_on)
    assert all(bool(torch.isfinite(v).all()) for v in loss_on)
    assert [v.item() for v in loss_on] == [v.item() for v in loss_off]
    diff = [k for k in sd_off if not torch.equal(sd_off[k], sd_on[k])]
    assert not diff, diff
    _check_arms(p_off, p_on, arm)
