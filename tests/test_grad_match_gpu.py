"""mdemi.functional.grad_match_loss (csrc/gradmatch.hip) against the fp64 reference of
tests/grad_match_ref.py, forward and backward, at SILog's bars (test_kernels_gpu.py::test_silog):
loss rtol 1e-5, gradient rtol 1e-3 / atol 1e-7 of the largest reference gradient, and exactly 0
on invalid pixels.  Pixels of a pair with 0 < |dR| < 1e-5, whose sign an fp32 logf may
legitimately flip, are left out of the gradient check; they may be at most 1 % of the valid ones."""
import numpy as np
import pytest
import torch

from grad_match_ref import SHAPES, grad_match_ref, make_inputs, reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
MD = 1e-3


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32)).to(DEV)  # a copy: the shared inputs are read-only


def _run(mf, pred, gt, scales, per_image):
    pg = _dev(pred).unsqueeze(1).requires_grad_()
    loss = mf.grad_match_loss(pg, _dev(gt).unsqueeze(1), MD, scales, per_image)
    loss.backward()
    return loss.detach(), pg.grad[:, 0]


def _check(loss, grad, ref, gt, scale=1.0):
    lr, gr, tie = ref
    valid = gt > MD
    assert tie.sum() <= 0.01 * valid.sum(), (int(tie.sum()), int(valid.sum()))
    lg, gg = float(loss.double().cpu()), grad.double().cpu().numpy()
    print(f"loss {lg:.9g} ref {lr:.9g} rel.err {abs(lg - lr) / max(abs(lr), 1e-300):.3e}; "
          f"max|dgrad| {np.abs(gg - scale * gr)[~tie].max():.3e} of max|grad| {np.abs(gr).max():.3e}; "
          f"near-tie {int(tie.sum())}/{int(valid.sum())}")
    assert abs(lg - lr) <= 1e-5 * abs(lr)
    assert np.isfinite(gg).all() and (gg[~valid] == 0).all()
    err = np.abs(gg - scale * gr)[~tie].max()
    assert err <= 1e-7 + 1e-3 * scale * np.abs(gr).max(), err


@pytest.mark.parametrize("scales", [1, 4])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("B,H,W,keep", SHAPES)
def test_against_the_fp64_reference(mf, B, H, W, keep, per_image, scales):
    pred, gt = make_inputs(B, H, W, keep)
    loss, grad = _run(mf, pred, gt, scales, per_image)
    _check(loss, grad, reference(B, H, W, keep, scales, per_image), gt)


@pytest.mark.parametrize("per_image", [False, True])
def test_vector_path_across_tiles_and_unaligned_base(mf, per_image):
    """W % 4 == 0 takes the 4-pixel loads; 260 columns are three tiles, 40 rows two, so every halo
    (the rows and columns 1, 2, 4 and 8 before a tile) crosses a tile edge on that path.  The same
    tensors one float off 16-byte alignment take the scalar path and give the same bits."""
    B, H, W, keep = 2, 40, 260, 0.9
    pred, gt = make_inputs(B, H, W, keep)
    loss, grad = _run(mf, pred, gt, 4, per_image)
    _check(loss, grad, reference(B, H, W, keep, 4, per_image), gt)
    n = B * H * W
    pbuf, gbuf = torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV)
    pbuf[1:] = _dev(pred).reshape(-1)
    gbuf[1:] = _dev(gt).reshape(-1)
    po = pbuf[1:].view(B, 1, H, W).requires_grad_()
    assert po.is_contiguous() and po.data_ptr() % 16 == 4
    lo = mf.grad_match_loss(po, gbuf[1:].view(B, 1, H, W), MD, 4, per_image)
    lo.backward()
    assert torch.equal(lo.detach(), loss) and torch.equal(po.grad[:, 0], grad)


def test_upstream_gradient_and_three_dim_inputs(mf):
    """dloss scales the gradient; (B,H,W) tensors are taken as they are."""
    B, H, W, keep = SHAPES[0]
    pred, gt = make_inputs(B, H, W, keep)
    pg = _dev(pred).requires_grad_()
    loss = mf.grad_match_loss(pg, _dev(gt), MD, 3, True)
    (loss * 0.25).backward()
    _check(loss.detach(), pg.grad, grad_match_ref(pred, gt, MD, 3, True), gt, scale=0.25)


def test_scale_invariance(mf):
    """The term does not see pred -> c * pred: both losses meet the loss bar against one reference."""
    B, H, W, keep = SHAPES[0]
    pred, gt = make_inputs(B, H, W, keep)
    l1, _ = _run(mf, pred, gt, 4, False)
    l4, g4 = _run(mf, 4.0 * pred, gt, 4, False)  # 4 * pred is exact in fp32
    assert abs(float(l4) - float(l1)) <= 1e-5 * float(l1)
    _check(l4, g4, grad_match_ref(4.0 * pred, gt, MD, 4, False), gt)


@pytest.mark.parametrize("per_image", [False, True])
def test_constant_inputs_give_exactly_zero(mf, per_image):
    """Every pair difference is 0: sign(0) = 0, so no pixel gets a gradient."""
    pred = np.full((2, 19, 41), 2.5, np.float32)
    gt = np.full((2, 19, 41), 4.0, np.float32)
    loss, grad = _run(mf, pred, gt, 4, per_image)
    assert float(loss) == 0.0 and not grad.any().item()


@pytest.mark.parametrize("per_image", [False, True])
def test_all_invalid_ground_truth(mf, per_image):
    pred, _ = make_inputs(*SHAPES[0])
    gt = np.zeros_like(pred)
    loss, grad = _run(mf, pred, gt, 4, per_image)
    assert float(loss) == 0.0 and torch.isfinite(grad).all().item() and not grad.any().item()
    # one image without a valid pixel beside one with: it leaves the per-image mean
    pred, gt = make_inputs(*SHAPES[3])
    gt = gt.copy()
    gt[1] = 0.0
    loss, grad = _run(mf, pred, gt, 4, per_image)
    _check(loss, grad, grad_match_ref(pred, gt, MD, 4, per_image), gt)
    assert not grad[1].any().item()


def test_two_runs_are_bit_identical(mf):
    for shape in (SHAPES[0], SHAPES[2]):
        pred, gt = make_inputs(*shape)
        l1, g1 = _run(mf, pred, gt, 4, True)
        l2, g2 = _run(mf, pred, gt, 4, True)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_non_contiguous_prediction(mf):
    B, H, W, keep = SHAPES[0]
    pred, gt = make_inputs(B, H, W, keep)
    wide = torch.zeros(B, 1, H, 2 * W, device=DEV)
    wide[..., ::2] = _dev(pred).unsqueeze(1)
    wide.requires_grad_()
    view = wide[..., ::2]
    assert not view.is_contiguous()
    g = _dev(gt).unsqueeze(1)
    loss = mf.grad_match_loss(view, g, MD, 4, False)
    loss.backward()
    l2, g2 = _run(mf, pred, gt, 4, False)
    assert torch.equal(loss.detach(), l2) and torch.equal(wide.grad[:, 0, :, ::2], g2)
    assert not wide.grad[..., 1::2].any().item()


def test_bad_arguments_raise_before_anything_is_launched(mf):
    from mdemi import _lib
    from mdemi.train import TrainLoss
    x = torch.ones(1, 1, 8, 8, device=DEV)
    for bad in (5, 0):
        with pytest.raises(ValueError, match="scales"):
            mf.grad_match_loss(x, x, scales=bad)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="loss.grad_weight"):
            TrainLoss({"loss": {"grad_weight": bad}}, "newcrfs")
    # the C ABI refuses them too, with the usual codes and without a launch
    lib = _lib.load()
    assert lib.mdemi_gradmatch_workspace_size(2, 37, 70) >= 2 * 2 * 8 * 4
    rc = lib.mdemi_gradmatch_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, 8, MD, 5, 0,
                                 x.data_ptr(), None)
    assert rc < 0 and b"scales" in lib.mdemi_last_error()
    assert lib.mdemi_gradmatch_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, 8, MD, 4, 0,
                                   None, None) < 0
    assert lib.mdemi_gradmatch_fwd(None, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, 8, MD, 4, 0,
                                   x.data_ptr(), None) < 0
    assert lib.mdemi_gradmatch_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1, 8, 8, MD, 4,
                                   None) < 0
    assert lib.mdemi_gradmatch_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 0, 8, MD,
                                   4, None) < 0
