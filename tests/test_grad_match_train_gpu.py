"""The gradient-matching term inside the config-driven train step (loss.grad_weight): the tiny07
NeW-CRFs at 64x96, batch 2, as tests/test_run_gpu.py configures it.  Off, the step is bit for bit
the step without the key; on, the loss is silog + weight x the term on the same prediction; the
hipGraph-captured step equals the eager one; a half-resolution prediction is resized once."""
import copy

import numpy as np
import pytest
import torch

from grad_match_ref import grad_match_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


def _opt(**loss):
    return {"model": {"name": "newcrfs", "version": "tiny07"},
            "loss": {"alpha": 10.0, "beta": 0.15, "per_image": False, **loss},
            "dataset": {"data_type": "NYU", "img_size": [64, 96]}, "dataloader": {"batch_size": 2},
            "optimizer": {"lr": 2e-4, "weight_decay": 0.01},
            "scheduler": {"name": "onecycle", "pct_start": 0.3, "div_factor": 25, "final_div_factor": 100},
            "train": {"epoch": 2, "num_accum": 1, "grad_norm": 0.1},
            "eval": {"max_depth_eval": 10, "min_depth_eval": 0.001}}


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(2, 3, 64, 96, generator=g)
    gt = torch.rand(2, 1, 64, 96, generator=g) * 9.5 + 0.5
    gt[:, :, :5] = 0.0
    return img.to(DEV), gt.to(DEV)


def _trainer(opt, state=None, **kw):
    from mdemi.train import build_from_config
    torch.manual_seed(0)
    t = build_from_config(copy.deepcopy(opt), device=DEV, steps_per_epoch=20, drop_path=0.0, **kw)
    if state is not None:
        t.model.load_state_dict(state)
    return t


@pytest.fixture(scope="module")
def plain(mf):
    """The trainer without the key, its initial weights, and its first step's loss."""
    t = _trainer(_opt())
    state = copy.deepcopy(t.model.state_dict())
    loss = t.step([_batch(0)]).clone()
    return t, state, loss


def test_weight_zero_is_the_step_without_the_key(mf, plain):
    t0, state, loss0 = plain
    assert t0.criterion.grad is None
    tz = _trainer(_opt(grad_weight=0.0), state)
    assert tz.criterion.grad is None
    lz = tz.step([_batch(0)])
    assert torch.equal(lz, loss0), (lz.item(), loss0.item())
    for (k, a), b in zip(t0.model.state_dict().items(), tz.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_weighted_sum_of_the_two_terms(mf, plain):
    from mdemi.train import GradMatchLoss
    _, state, loss0 = plain
    tw = _trainer(_opt(grad_weight=0.5), state)
    assert isinstance(tw.criterion.grad, GradMatchLoss) and tw.criterion.grad.scales == 4
    img, gt = _batch(0)
    tw.train_mode()
    with torch.no_grad():
        pred = tw.model(img)
    silog = mf.silog_loss(pred, gt, 1e-3, 10.0, 0.15, False)
    gm = mf.grad_match_loss(pred, gt, 1e-3, 4, False)
    assert torch.equal(silog, loss0) and gm.item() > 0
    # the term against the fp64 reference on this prediction, at the kernel test's loss bar
    ref = grad_match_ref(pred[:, 0].double().cpu().numpy(), gt[:, 0].double().cpu().numpy(), 1e-3, 4, False)[0]
    assert abs(gm.item() - ref) <= 1e-5 * ref
    loss = tw.step([(img, gt)])
    assert torch.equal(loss, silog + 0.5 * gm), (loss.item(), silog.item(), gm.item())


def test_graph_captured_step_matches_eager(mf, plain):
    _, state, _ = plain
    opt = _opt(grad_weight=0.5, grad_scales=3, per_image=True)
    eager = _trainer(opt, state)
    graph = _trainer(opt, state, graph=True)
    batches = [_batch(s) for s in range(4)]
    le, lg = [], []
    for b in batches:  # graph: calls 1-2 run eagerly (warm-up), 3 captures + replays, 4 replays
        le.append(eager.step([b]).item())
        lg.append(graph.step([b]).item())
    assert graph._graph is not None
    assert le == lg, (le, lg)
    assert len(set(le)) == 4 and all(np.isfinite(le))
    for (k, a), b in zip(eager.model.state_dict().items(), graph.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_oda2_averages_the_term_over_every_output(mf):
    """ODA2 returns (out, outs, attn): the term is averaged over outs exactly as si_weight x SILog is,
    each output resized to the GT; without the weight the loss is the SILog average alone."""
    from mdemi.train import TrainLoss
    from mdemi.train.loss import resize_to_gt
    g = torch.Generator().manual_seed(12)
    gt = torch.rand(2, 1, 32, 48, generator=g) * 9.5 + 0.5
    gt[:, :, :3] = 0.0
    gt = gt.to(DEV)
    outs = [(torch.rand(2, 1, 32, 48, generator=g) * 9.0 + 0.5).to(DEV),
            (torch.rand(2, 1, 16, 24, generator=g) * 9.0 + 0.5).to(DEV),
            (torch.rand(2, 1, 8, 12, generator=g) * 9.0 + 0.5).to(DEV)]
    full = [resize_to_gt(o, gt) for o in outs]
    si = mf.silog_loss(full[0], gt, 1e-3, 10.0, 0.15, False)
    gm = mf.grad_match_loss(full[0], gt, 1e-3, 2, False)
    for f in full[1:]:
        si = si + mf.silog_loss(f, gt, 1e-3, 10.0, 0.15, False)
        gm = gm + mf.grad_match_loss(f, gt, 1e-3, 2, False)
    plain = TrainLoss(_opt(si_weight=0.7), "oda2_red_order_swin2")((outs[0], outs, None), gt)
    assert torch.equal(plain, si * (0.7 / 3))
    crit = TrainLoss(_opt(si_weight=0.7, grad_weight=0.5, grad_scales=2), "oda2_red_order_swin2")
    assert torch.equal(crit((outs[0], outs, None), gt), si * (0.7 / 3) + gm * (0.5 / 3))
    refs = [grad_match_ref(f[:, 0].double().cpu().numpy(), gt[:, 0].double().cpu().numpy(), 1e-3, 2, False)[0]
            for f in full]
    assert abs(gm.item() - sum(refs)) <= 1e-5 * sum(refs)


@pytest.mark.parametrize("name", ["adabins", "depthformer_v8"])
def test_half_resolution_prediction_is_resized_once(mf, name):
    from mdemi.train import TrainLoss
    from mdemi.train.loss import resize_to_gt
    opt = _opt(grad_weight=0.5, per_image=True)
    opt["loss"]["beta"] = 0.5
    crit = TrainLoss(opt, name)
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(2, 1, 32, 48, generator=g) * 9.5 + 0.5
    gt[:, :, :3] = 0.0
    gt = gt.to(DEV)
    half = (torch.rand(2, 1, 16, 24, generator=g) * 9.0 + 0.5).to(DEV).requires_grad_()
    full = resize_to_gt(half.detach(), gt)
    assert full.shape == gt.shape
    calls = []
    orig = mf.interpolate_bilinear

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    mf.interpolate_bilinear = counted
    try:
        loss = crit((half, None), gt)  # (depth, bins): no chamfer weight, the bins are not read
    finally:
        mf.interpolate_bilinear = orig
    assert len(calls) == 1
    silog = mf.silog_loss(full, gt, 1e-3, 10.0, 0.5, True)
    ref, gref, tie = grad_match_ref(full[:, 0].double().cpu().numpy(), gt[:, 0].double().cpu().numpy(), 1e-3, 4, True)
    want = silog.item() + 0.5 * ref
    assert abs(loss.item() - want) <= 1e-5 * want
    assert torch.equal(loss, silog + 0.5 * mf.grad_match_loss(full, gt, 1e-3, 4, True))
    # the gradient reaches the half-resolution prediction through the one resize
    loss.backward()
    f2 = full.clone().requires_grad_()
    (mf.silog_loss(f2, gt, 1e-3, 10.0, 0.5, True) + 0.5 * mf.grad_match_loss(f2, gt, 1e-3, 4, True)).backward()
    h2 = half.detach().clone().requires_grad_()
    resize_to_gt(h2, gt).backward(f2.grad)
    assert torch.equal(half.grad, h2.grad) and half.grad.abs().max().item() > 0
    # SILogLoss on its own still resizes a half-resolution prediction itself
    assert torch.equal(crit.silog(half.detach(), gt), silog)
