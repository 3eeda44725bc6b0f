"""The scale- and shift-invariant term inside the config-driven train step (loss.ssi_weight): the
tiny07 NeW-CRFs at 64x96, batch 2, as tests/test_grad_match_train_gpu.py configures it.  Off, the
step is bit for bit the step without the key; on, the loss is silog + weight x the term on the same
prediction; si_weight 0 leaves the term alone; the hipGraph-captured step equals the eager one."""
import copy

import numpy as np
import pytest
import torch

from ssi_ref import ssi_ref

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


def _np(t):
    return t[:, 0].double().cpu().numpy()


@pytest.fixture(scope="module")
def plain(mf):
    """The trainer without the key, its initial weights, its first step's loss and the prediction
    that step saw."""
    t = _trainer(_opt())
    state = copy.deepcopy(t.model.state_dict())
    img, gt = _batch(0)
    loss = t.step([(img, gt)]).clone()
    tp = _trainer(_opt(), state)  # a second model: t's buffers see exactly one forward
    tp.train_mode()
    with torch.no_grad():
        pred = tp.model(img).clone()
    return t, state, loss, pred


def test_weight_zero_is_the_step_without_the_key(mf, plain):
    t0, state, loss0, _ = plain
    assert t0.criterion.ssi is None
    tz = _trainer(_opt(ssi_weight=0.0, ssi_space="disp", ssi_trim=0.2, si_weight=0.3), state)
    assert tz.criterion.ssi is None  # and si_weight is not read on this path while the term is off
    lz = tz.step([_batch(0)])
    assert torch.equal(lz, loss0), (lz.item(), loss0.item())
    for (k, a), b in zip(t0.model.state_dict().items(), tz.model.state_dict().values()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("space,trim,norm", [("depth", 0.0, "none"), ("disp", 0.2, "gt_var")])
def test_weighted_sum_of_the_two_terms(mf, plain, space, trim, norm):
    from mdemi.train import SSILoss
    _, state, loss0, pred = plain
    tw = _trainer(_opt(ssi_weight=0.5, ssi_space=space, ssi_trim=trim, ssi_norm=norm), state)
    assert isinstance(tw.criterion.ssi, SSILoss) and tw.criterion.ssi.space == space
    img, gt = _batch(0)
    silog = mf.silog_loss(pred, gt, 1e-3, 10.0, 0.15, False)
    ssi = mf.ssi_loss(pred, gt, 1e-3, space, trim, norm, False)
    assert torch.equal(silog, loss0) and ssi.item() > 0
    # the term against the fp64 reference on this prediction, at the kernel test's loss bar
    ref = ssi_ref(_np(pred), _np(gt), 1e-3, space, trim, norm, False)[0]
    print(f"ssi {ssi.item():.9g} ref {ref:.9g} rel.err {abs(ssi.item() - ref) / ref:.3e}")
    assert abs(ssi.item() - ref) <= 1e-5 * ref
    loss = tw.step([(img, gt)])
    assert torch.equal(loss, silog + 0.5 * ssi), (loss.item(), silog.item(), ssi.item())


def test_si_weight_zero_leaves_exactly_the_term(mf, plain):
    _, state, _, pred = plain
    img, gt = _batch(0)
    ts = _trainer(_opt(si_weight=0, ssi_weight=1.0, ssi_space="disp"), state)
    calls = []
    orig = mf.silog_loss

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    mf.silog_loss = counted
    try:
        loss = ts.step([(img, gt)])
    finally:
        mf.silog_loss = orig
    assert not calls  # no SILog was launched
    assert torch.equal(loss, 1.0 * mf.ssi_loss(pred, gt, 1e-3, "disp", 0.0, "none", False))
    # a fractional si_weight weighs SILog on this single-output model while the term is on
    th = _trainer(_opt(si_weight=0.25, ssi_weight=1.0), state)
    want = 0.25 * mf.silog_loss(pred, gt, 1e-3, 10.0, 0.15, False) + 1.0 * mf.ssi_loss(pred, gt, 1e-3)
    assert torch.equal(th.step([(img, gt)]), want)


def test_graph_captured_step_matches_eager(mf, plain):
    _, state, _, _ = plain
    opt = _opt(ssi_weight=0.5, ssi_trim=0.2, ssi_space="disp", per_image=True)
    eager = _trainer(opt, state)
    graph = _trainer(opt, state, graph=True)
    batches = [_batch(s) for s in range(4)]
    le, lg = [], []
    for b in batches:  # graph: calls 1-2 run eagerly (warm-up), 3 captures + replays, 4 replays
        le.append(eager.step([b]).clone())
        lg.append(graph.step([b]).clone())
    assert graph._graph is not None
    assert all(torch.equal(a, b) for a, b in zip(le, lg)), (le, lg)
    assert len({x.item() for x in le}) == 4 and all(np.isfinite(x.item()) for x in le)
    for (k, a), b in zip(eager.model.state_dict().items(), graph.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_oda2_averages_the_term_over_every_output(mf):
    """ODA2 returns (out, outs, attn): the term is averaged over outs exactly as si_weight x SILog and
    the gradient term are, each output resized to the GT; all three terms sum."""
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

    def total(fn):
        acc = fn(full[0])
        for f in full[1:]:
            acc = acc + fn(f)
        return acc

    si = total(lambda f: mf.silog_loss(f, gt, 1e-3, 10.0, 0.15, False))
    gm = total(lambda f: mf.grad_match_loss(f, gt, 1e-3, 2, False))
    ssi = total(lambda f: mf.ssi_loss(f, gt, 1e-3, "depth", 0.2, "gt_var", False))
    kw = dict(ssi_weight=0.4, ssi_trim=0.2, ssi_norm="gt_var")
    crit = TrainLoss(_opt(si_weight=0.7, **kw), "oda2_red_order_swin2")
    assert torch.equal(crit((outs[0], outs, None), gt), si * (0.7 / 3) + ssi * (0.4 / 3))
    crit = TrainLoss(_opt(si_weight=0.7, grad_weight=0.5, grad_scales=2, **kw), "oda2_red_order_swin2")
    assert torch.equal(crit((outs[0], outs, None), gt), si * (0.7 / 3) + gm * (0.5 / 3) + ssi * (0.4 / 3))
    crit = TrainLoss(_opt(si_weight=0, **kw), "oda2_red_order_swin2")
    assert torch.equal(crit((outs[0], outs, None), gt), ssi * (0.4 / 3))
    refs = [ssi_ref(_np(f), _np(gt), 1e-3, "depth", 0.2, "gt_var", False)[0] for f in full]
    assert abs(ssi.item() - sum(refs)) <= 1e-5 * sum(refs)


def test_the_three_terms_sum_on_a_half_resolution_prediction(mf):
    """With grad_weight too the loss is silog + grad_weight x gm + ssi_weight x ssi, on the one resize."""
    from mdemi.train import TrainLoss
    from mdemi.train.loss import resize_to_gt
    crit = TrainLoss(_opt(grad_weight=0.5, ssi_weight=0.25, ssi_space="disp", per_image=True), "adabins")
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(2, 1, 32, 48, generator=g) * 9.5 + 0.5
    gt[:, :, :3] = 0.0
    gt = gt.to(DEV)
    half = (torch.rand(2, 1, 16, 24, generator=g) * 9.0 + 0.5).to(DEV).requires_grad_()
    full = resize_to_gt(half.detach(), gt)
    calls = []
    orig = mf.interpolate_bilinear

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    mf.interpolate_bilinear = counted
    try:
        loss = crit((half, None), gt)
    finally:
        mf.interpolate_bilinear = orig
    assert len(calls) == 1

    def terms(f):
        return mf.silog_loss(f, gt, 1e-3, 10.0, 0.15, True) + 0.5 * mf.grad_match_loss(f, gt, 1e-3, 4, True) + \
            0.25 * mf.ssi_loss(f, gt, 1e-3, "disp", 0.0, "none", True)

    assert torch.equal(loss, terms(full))
    loss.backward()
    f2 = full.clone().requires_grad_()
    terms(f2).backward()
    h2 = half.detach().clone().requires_grad_()
    resize_to_gt(h2, gt).backward(f2.grad)
    assert torch.equal(half.grad, h2.grad) and half.grad.abs().max().item() > 0
