"""mdemi.functional.ssi_loss (csrc/ssi.hip) against the fp64 reference of tests/ssi_ref.py, forward
and backward, at SILog's and the gradient term's bars (test_grad_match_gpu.py): loss rtol 1e-5,
gradient 1e-7 + 1e-3 of the largest reference gradient, and exactly 0 on invalid pixels.  Pixels
whose rho lies within 1e-5 tau of tau, whose side a last-bit difference in (s, t) may legitimately
change, are left out of the gradient check; they may be at most 1 % of the valid ones."""
import numpy as np
import pytest
import torch

from ssi_ref import NORMS, SHAPES, SPACES, make_inputs, reference, ssi_ref

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


def _run(mf, pred, gt, space="depth", trim=0.0, norm="none", per_image=False):
    pg = _dev(pred).unsqueeze(1).requires_grad_()
    loss = mf.ssi_loss(pg, _dev(gt).unsqueeze(1), MD, space, trim, norm, per_image)
    loss.backward()
    return loss.detach(), pg.grad[:, 0]


def _check(loss, grad, ref, gt, scale=1.0):
    lr, gr, near = ref
    valid = gt > MD
    assert near.sum() <= 0.01 * valid.sum(), (int(near.sum()), int(valid.sum()))
    lg, gg = float(loss.double().cpu()), grad.double().cpu().numpy()
    print(f"loss {lg:.9g} ref {lr:.9g} rel.err {abs(lg - lr) / max(abs(lr), 1e-300):.3e}; "
          f"max|dgrad| {np.abs(gg - scale * gr)[~near].max():.3e} of max|grad| {np.abs(gr).max():.3e}; "
          f"near-tau {int(near.sum())}/{int(valid.sum())}")
    assert abs(lg - lr) <= 1e-5 * abs(lr)
    assert np.isfinite(gg).all() and (gg[~valid] == 0).all()
    err = np.abs(gg - scale * gr)[~near].max()
    assert err <= 1e-7 + 1e-3 * scale * np.abs(gr).max(), err


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("trim", [0.0, 0.2])
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("B,H,W,keep", SHAPES)
def test_against_the_fp64_reference(mf, B, H, W, keep, space, trim, per_image, norm):
    """The shapes cover a single chunk with a small u (2, 5, 7), sparse ground truth (2, 33, 130),
    an odd pixel count (3, 37, 70: the scalar path) and the vector path over several chunks (2, 40, 260)."""
    pred, gt = make_inputs(B, H, W, keep)
    loss, grad = _run(mf, pred, gt, space, trim, norm, per_image)
    _check(loss, grad, reference(B, H, W, keep, space, trim, norm, per_image), gt)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("trim", [0.0, 0.2])
def test_base_one_float_off_alignment(mf, space, trim):
    """(2, 40, 260) takes the 4-pixel loads; the same tensors one float off 16-byte alignment take
    the scalar path and meet the same bars."""
    B, H, W, keep = 2, 40, 260, 0.9
    pred, gt = make_inputs(B, H, W, keep)
    n = B * H * W
    pbuf, gbuf = torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV)
    pbuf[1:] = _dev(pred).reshape(-1)
    gbuf[1:] = _dev(gt).reshape(-1)
    po = pbuf[1:].view(B, 1, H, W).requires_grad_()
    assert po.is_contiguous() and po.data_ptr() % 16 == 4
    lo = mf.ssi_loss(po, gbuf[1:].view(B, 1, H, W), MD, space, trim, "none", True)
    lo.backward()
    _check(lo.detach(), po.grad[:, 0], reference(B, H, W, keep, space, trim, "none", True), gt)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("trim", [0.0, 0.2])
def test_exact_fit_gives_a_vanishing_loss(mf, space, trim):
    pred, gt = make_inputs(*SHAPES[0])
    loss, grad = _run(mf, np.where(gt > MD, gt, pred), gt, space, trim)
    assert 0.0 <= float(loss) < 1e-20 and torch.isfinite(grad).all().item()


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("space", SPACES)
def test_constant_prediction_is_skipped(mf, space, per_image):
    """pred == 2 everywhere: n Sxx - Sx^2 is exactly 0 in both spaces.  Alone the image gives loss 0
    and gradient exactly 0; beside a good image it leaves both reductions."""
    pred, gt = make_inputs(*SHAPES[0])
    flat = np.full_like(pred[:1], 2.0)
    for trim in (0.0, 0.2):
        loss, grad = _run(mf, flat, gt[:1], space, trim, "none", per_image)
        assert float(loss) == 0.0 and not grad.any().item()
        p = pred.copy()
        p[1] = 2.0
        loss, grad = _run(mf, p, gt, space, trim, "gt_var", per_image)
        _check(loss, grad, ssi_ref(p, gt, MD, space, trim, "gt_var", per_image), gt)
        assert not grad[1].any().item()


@pytest.mark.parametrize("per_image", [False, True])
def test_one_and_two_valid_pixels_and_none(mf, per_image):
    pred, gt = make_inputs(*SHAPES[0])
    for trim in (0.0, 0.2):
        # n == 1: det == 0, skipped
        g = np.zeros_like(gt)
        g[:, 5, 5] = 2.0
        loss, grad = _run(mf, pred, g, "depth", trim, "none", per_image)
        assert float(loss) == 0.0 and not grad.any().item()
        # n == 2: the line through two points, residuals at fp64 rounding
        g[:, 9, 60] = 5.0
        assert ((g > MD).reshape(3, -1).sum(1) == 2).all() and (pred[:, 5, 5] != pred[:, 9, 60]).all()
        loss, grad = _run(mf, pred, g, "depth", trim, "none", per_image)
        assert 0.0 <= float(loss) < 1e-20 and torch.isfinite(grad).all().item()
        assert not grad[torch.from_numpy(g <= MD).to(DEV)].any().item()
        # no valid pixel anywhere
        loss, grad = _run(mf, pred, np.zeros_like(gt), "depth", trim, "none", per_image)
        assert float(loss) == 0.0 and torch.isfinite(grad).all().item() and not grad.any().item()
    # one image without a valid pixel beside two with: it leaves the per-image mean
    g = gt.copy()
    g[1] = 0.0
    loss, grad = _run(mf, pred, g, "disp", 0.2, "gt_var", per_image)
    _check(loss, grad, ssi_ref(pred, g, MD, "disp", 0.2, "gt_var", per_image), g)
    assert not grad[1].any().item()


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("trim", [0.0, 0.2])
def test_nan_prediction_on_a_valid_pixel_gives_a_nan_loss(mf, trim, per_image):
    pred, gt = make_inputs(*SHAPES[0])
    p = pred.copy()
    y, x = np.argwhere(gt[1] > MD)[7]
    p[1, y, x] = np.nan
    loss, grad = _run(mf, p, gt, "depth", trim, "none", per_image)
    assert torch.isnan(loss).item()
    assert not grad[torch.from_numpy(gt <= MD).to(DEV)].any().item()  # still exactly 0 off V
    # pred == 0 under disp is the same; the same pixels off V change nothing
    p[1, y, x] = 0.0
    assert torch.isnan(_run(mf, p, gt, "disp", trim, "none", per_image)[0]).item()
    p = pred.copy()
    y, x = np.argwhere(gt[1] <= MD)[7]
    p[1, y, x] = np.nan
    loss, grad = _run(mf, p, gt, "depth", trim, "none", per_image)
    l0, g0 = _run(mf, pred, gt, "depth", trim, "none", per_image)
    assert torch.equal(loss, l0) and torch.equal(grad, g0)


@pytest.mark.parametrize("space", SPACES)
def test_trim_one_half(mf, space):
    for shape in (SHAPES[0], SHAPES[1]):
        pred, gt = make_inputs(*shape)
        loss, grad = _run(mf, pred, gt, space, 0.5, "gt_var", True)
        _check(loss, grad, reference(*shape, space, 0.5, "gt_var", True), gt)


def test_ties_at_tau_are_all_kept(mf):
    """Residuals of exactly +-1 and 0 (s = 1, t = 0 exactly): tau = 1 and all ten pixels stay."""
    x = np.arange(10, dtype=np.float32) + 1
    off = np.array([1, -1, 1, -1, 0, 0, -1, 1, -1, 1], np.float32)
    pred, gt = x.reshape(1, 2, 5), (x + off).reshape(1, 2, 5)
    ref = ssi_ref(pred, gt, MD, "depth", 0.3)
    assert abs(ref[0] - 8.0 / 20.0) < 1e-12  # Q = 8, U = 10
    loss, grad = _run(mf, pred, gt, "depth", 0.3)
    lg = float(loss)
    assert abs(lg - ref[0]) <= 1e-5 * ref[0]
    gg = grad.double().cpu().numpy()
    assert np.abs(gg - ref[1]).max() <= 1e-7 + 1e-3 * np.abs(ref[1]).max()


def test_upstream_gradient_and_three_dim_inputs(mf):
    """dloss scales the gradient; (B,H,W) tensors are taken as they are."""
    B, H, W, keep = SHAPES[0]
    pred, gt = make_inputs(B, H, W, keep)
    pg = _dev(pred).requires_grad_()
    loss = mf.ssi_loss(pg, _dev(gt), MD, "disp", 0.2, "gt_var", True)
    (loss * 0.25).backward()
    _check(loss.detach(), pg.grad, reference(B, H, W, keep, "disp", 0.2, "gt_var", True), gt, scale=0.25)


def test_two_runs_are_bit_identical(mf):
    for shape in (SHAPES[0], SHAPES[4]):
        pred, gt = make_inputs(*shape)
        for trim in (0.0, 0.2):
            l1, g1 = _run(mf, pred, gt, "disp", trim, "gt_var", True)
            l2, g2 = _run(mf, pred, gt, "disp", trim, "gt_var", True)
            assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_non_contiguous_prediction(mf):
    B, H, W, keep = SHAPES[0]
    pred, gt = make_inputs(B, H, W, keep)
    wide = torch.zeros(B, 1, H, 2 * W, device=DEV)
    wide[..., ::2] = _dev(pred).unsqueeze(1)
    wide.requires_grad_()
    view = wide[..., ::2]
    assert not view.is_contiguous()
    loss = mf.ssi_loss(view, _dev(gt).unsqueeze(1), MD, "depth", 0.2)
    loss.backward()
    l2, g2 = _run(mf, pred, gt, "depth", 0.2)
    assert torch.equal(loss.detach(), l2) and torch.equal(wide.grad[:, 0, :, ::2], g2)
    assert not wide.grad[..., 1::2].any().item()


def test_the_c_abi_refuses_bad_arguments_without_a_launch(mf):
    from mdemi import _lib
    lib = _lib.load()
    x = torch.ones(1, 1, 8, 8, device=DEV)
    out = torch.full((16,), 7.0, device=DEV, dtype=torch.float64)  # loss / coef: must stay untouched
    ws = torch.zeros(lib.mdemi_ssi_workspace_size(1, 8, 8, 1) // 4 + 4, dtype=torch.int32, device=DEV)
    assert lib.mdemi_ssi_workspace_size(1, 8, 8, 1) >= lib.mdemi_ssi_workspace_size(1, 8, 8, 0) + 64 * 4 + 2048 * 4
    assert lib.mdemi_ssi_workspace_size(0, 8, 8, 0) == 0
    p, o, w = x.data_ptr(), out.data_ptr(), ws.data_ptr()

    def fwd(pred=p, gt=p, loss=o, coef=o + 8, B=1, H=8, W=8, space=0, trim=0.2, norm=0, workspace=w):
        return lib.mdemi_ssi_fwd(pred, gt, loss, coef, B, H, W, MD, space, trim, norm, 0, workspace, None)

    def bwd(pred=p, gt=p, coef=o + 8, dloss=p, dpred=p, B=1, H=8, W=8, space=0):
        return lib.mdemi_ssi_bwd(pred, gt, coef, dloss, dpred, B, H, W, MD, space, None)

    cases = [(fwd, dict(B=0), b"B"), (fwd, dict(B=65536), b"B"), (fwd, dict(space=2), b"space"),
             (fwd, dict(space=-1), b"space"), (fwd, dict(norm=2), b"norm"), (fwd, dict(trim=-0.1), b"trim"),
             (fwd, dict(trim=0.6), b"trim"), (fwd, dict(trim=float("nan")), b"trim"),
             (fwd, dict(trim=float("inf")), b"trim"), (fwd, dict(workspace=None), b"workspace"),
             (fwd, dict(pred=None), b"pred"), (fwd, dict(gt=None), b"gt"), (fwd, dict(loss=None), b"loss"),
             (fwd, dict(coef=None), b"coef"), (fwd, dict(H=0), b"H"),
             (bwd, dict(B=0), b"B"), (bwd, dict(B=65536), b"B"), (bwd, dict(space=2), b"space"),
             (bwd, dict(coef=None), b"coef"), (bwd, dict(dloss=None), b"dloss"), (bwd, dict(dpred=None), b"dpred"),
             (bwd, dict(W=0), b"W")]
    for fn, kw, key in cases:
        rc = fn(**kw)
        assert rc < 0 and key in lib.mdemi_last_error(), (kw, rc, lib.mdemi_last_error())
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and not ws.any().item() and (x == 1).all().item()  # nothing ran
    assert fwd() == 0 and bwd() == 0  # and the good call goes through
    torch.cuda.synchronize()
    # Python refuses the same before the library is reached
    for kw in (dict(space="log"), dict(trim=0.6), dict(norm="mad")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            mf.ssi_loss(x, x, **kw)
