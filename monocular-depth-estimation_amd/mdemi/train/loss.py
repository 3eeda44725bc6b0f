"""SILog loss (restated; config keys loss.alpha / loss.beta / loss.per_image) and
the AdaBins bin chamfer loss (config key loss.chamfer_weight; restated from
upstream AdaBins' BinsChamferLoss -- the reference's loss module is absent).
AdaBins / Depthformer predictions are at half resolution and are resized to
the ground truth with bilinear align_corners=True first (upstream AdaBins
convention; parity unpinned).  The multi-scale gradient-matching loss (config keys
loss.grad_weight / loss.grad_scales) and the scale- and shift-invariant loss (loss.ssi_weight /
ssi_space / ssi_trim / ssi_norm) are this framework's own terms."""
import torch.nn as nn

from .. import functional as mf


def resize_to_gt(pred, gt):
    """pred (B,1,h,w) at the resolution of gt (B,1,H,W): itself when they agree, else bilinear
    align_corners=True."""
    if pred.shape[-2:] == gt.shape[-2:]:
        return pred
    B, _, h, w = pred.shape
    return mf.interpolate_bilinear(pred.reshape(B, h, w, 1), size=tuple(gt.shape[-2:]),
                                   align_corners=True).reshape(B, 1, *gt.shape[-2:])


class SILogLoss(nn.Module):
    def __init__(self, alpha=10.0, beta=0.15, per_image=False, min_depth=1e-3, unbiased=False):
        super().__init__()
        self.alpha, self.beta, self.per_image = float(alpha), float(beta), bool(per_image)
        self.min_depth, self.unbiased = float(min_depth), bool(unbiased)

    def forward(self, pred, gt):
        """pred (B,1,h,w), gt (B,1,H,W) NCHW (C=1, so also NHWC)."""
        return mf.silog_loss(resize_to_gt(pred, gt), gt, self.min_depth, self.alpha, self.beta, self.per_image,
                             self.unbiased)


class GradMatchLoss(nn.Module):
    """Multi-scale, scale-invariant gradient-matching loss (MegaDepth / MiDaS / DPT): over
    ``scales`` grids of step 1, 2, 4, 8 pixels, the absolute differences of log pred - log gt
    between adjacent valid grid pixels, normalised by the valid grid pixels -- per batch or
    per image, the switch SILog reads (one libmdemi sweep forward, one backward)."""

    def __init__(self, scales=4, per_image=False, min_depth=1e-3):
        super().__init__()
        self.scales, self.per_image = mf.check_grad_scales(scales), bool(per_image)
        self.min_depth = float(min_depth)

    def forward(self, pred, gt):
        """pred (B,1,h,w), gt (B,1,H,W); a half-resolution prediction is resized to the GT first."""
        return mf.grad_match_loss(resize_to_gt(pred, gt), gt, self.min_depth, self.scales, self.per_image)


class SSILoss(nn.Module):
    """Scale- and shift-invariant loss (MiDaS / DPT / Depth Anything's data term): per image, half
    the mean squared residual of the least-squares fit s x + t to y over the valid pixels, x and
    y the depths (``space`` "depth") or the inverse depths ("disp"); ``trim`` drops that share of
    the largest absolute residuals, ``norm`` "gt_var" divides by the variance of y -- per batch
    or per image, the switch SILog reads (config keys loss.ssi_*)."""

    def __init__(self, space="depth", trim=0.0, norm="none", per_image=False, min_depth=1e-3):
        super().__init__()
        self.space, self.trim, self.norm = mf.check_ssi_options(space, trim, norm)
        self.per_image, self.min_depth = bool(per_image), float(min_depth)

    def forward(self, pred, gt):
        """pred (B,1,h,w), gt (B,1,H,W); a half-resolution prediction is resized to the GT first."""
        return mf.ssi_loss(resize_to_gt(pred, gt), gt, self.min_depth, self.space, self.trim, self.norm,
                           self.per_image)


class BinsChamferLoss(nn.Module):
    """Chamfer distance between each image's bin centres and its valid (>= 1e-3) GT depths:
    mean over centres of the squared distance to the nearest depth plus mean over depths of
    the squared distance to the nearest centre, averaged over the batch (one libmdemi sweep
    forward, one backward)."""

    def __init__(self, thresh=1e-3, from_edges=True):
        super().__init__()
        self.thresh, self.from_edges = float(thresh), bool(from_edges)

    def forward(self, bins, gt):
        """bins: edges (B, P+1) (AdaBins), or centres (B, P, 1, 1) with from_edges=False
        (Depthformer v8)."""
        return mf.bins_chamfer(bins, gt, self.thresh, self.from_edges)
