"""Plain-numpy fp64 reference of the multi-scale gradient-matching loss and the
seeded inputs the GPU tests share.

R = log(pred) - log(gt) on M = gt > min_depth.  Scale k (step s = 2**k) works on R[::s, ::s]:
S_bk = sum of |R(y, x+s) - R(y, x)| and |R(y+s, x) - R(y, x)| over grid pairs valid at both ends,
N_bk = number of valid grid pixels.  Per batch L = sum_k sum_b S_bk / sum_b N_bk; per image
L = mean over images with N_b0 > 0 of sum_k S_bk / N_bk; an empty scale contributes 0."""
import functools

import numpy as np

TIE = 1e-5  # a pair with 0 < |dR| < TIE may legitimately change sign under an fp32 logf


def _scale_terms(R, M, s):
    """Of the scale-s grid: dx, mx, dy, my (pair differences and their validity)."""
    Rk, Mk = R[:, ::s, ::s], M[:, ::s, ::s]
    dx, mx = Rk[:, :, 1:] - Rk[:, :, :-1], Mk[:, :, 1:] & Mk[:, :, :-1]
    dy, my = Rk[:, 1:, :] - Rk[:, :-1, :], Mk[:, 1:, :] & Mk[:, :-1, :]
    return Mk, dx, mx, dy, my


def grad_match_sums(pred, gt, min_depth=1e-3, scales=4):
    """S[B, scales], N[B, scales] of the definition."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    M = gt > min_depth
    with np.errstate(all="ignore"):
        R = np.where(M, np.log(pred) - np.log(np.where(M, gt, 1.0)), 0.0)
    B = pred.shape[0]
    S, N = np.zeros((B, scales)), np.zeros((B, scales))
    for k in range(scales):
        Mk, dx, mx, dy, my = _scale_terms(R, M, 1 << k)
        S[:, k] = (np.abs(dx) * mx).reshape(B, -1).sum(1) + (np.abs(dy) * my).reshape(B, -1).sum(1)
        N[:, k] = Mk.reshape(B, -1).sum(1)
    return S, N


def grad_match_ref(pred, gt, min_depth=1e-3, scales=4, per_image=False):
    """pred, gt (B, H, W) -> (loss, dloss/dpred (B, H, W), near-tie mask (B, H, W)).  A near-tie
    pixel takes part in a valid pair of some scale with 0 < |dR| < TIE."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    assert pred.ndim == 3 and pred.shape == gt.shape
    B = pred.shape[0]
    M = gt > min_depth
    with np.errstate(all="ignore"):
        R = np.where(M, np.log(pred) - np.log(np.where(M, gt, 1.0)), 0.0)
    S, N = grad_match_sums(pred, gt, min_depth, scales)
    w = np.zeros((B, scales))  # dL/dS_bk
    if per_image:
        used = N[:, 0] > 0
        per = np.where(N > 0, S / np.where(N > 0, N, 1.0), 0.0).sum(1)
        loss = per[used].mean() if used.any() else 0.0
        ok = (N > 0) & used[:, None]
        w[ok] = 1.0 / (N[ok] * used.sum())
    else:
        Sk, Nk = S.sum(0), N.sum(0)
        loss = np.where(Nk > 0, Sk / np.where(Nk > 0, Nk, 1.0), 0.0).sum()
        w[:, Nk > 0] = 1.0 / Nk[Nk > 0]
    dR = np.zeros_like(R)
    tie = np.zeros(R.shape, bool)
    for k in range(scales):
        s = 1 << k
        _, dx, mx, dy, my = _scale_terms(R, M, s)
        c = np.zeros(R[:, ::s, ::s].shape)
        t = np.zeros(c.shape, bool)
        sx, sy = np.sign(dx) * mx, np.sign(dy) * my
        c[:, :, 1:] += sx
        c[:, :, :-1] -= sx
        c[:, 1:, :] += sy
        c[:, :-1, :] -= sy
        nx, ny = mx & (dx != 0) & (np.abs(dx) < TIE), my & (dy != 0) & (np.abs(dy) < TIE)
        t[:, :, 1:] |= nx
        t[:, :, :-1] |= nx
        t[:, 1:, :] |= ny
        t[:, :-1, :] |= ny
        dR[:, ::s, ::s] += w[:, k, None, None] * c
        tie[:, ::s, ::s] |= t
    grad = np.where(M, dR / np.where(M, pred, 1.0), 0.0)
    return float(loss), grad, tie


# (B, H, W, keep): odd sizes that cross tile edges; smaller than the largest step (scale 3 has one
# grid pixel and no pair); tile-aligned; KITTI-like sparse ground truth
SHAPES = [(3, 37, 70, 0.9), (2, 5, 7, 1.0), (1, 64, 96, 1.0), (2, 33, 130, 0.05)]


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, keep, seed=0):
    """(pred, gt) float32 (B, H, W): gt uniform in [0.5, 9.5], rows 0-2 and a random 1 - keep of the
    pixels invalid (0); pred = gt * exp(U(-0.5, 0.5)) where valid, an arbitrary positive value elsewhere."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 9.5, (B, H, W))
    gt[:, :3] = 0.0
    gt[rng.uniform(size=gt.shape) >= keep] = 0.0
    pred = np.where(gt > 0, gt * np.exp(rng.uniform(-0.5, 0.5, gt.shape)), rng.uniform(0.1, 10.0, gt.shape))
    pred, gt = pred.astype(np.float32), gt.astype(np.float32)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def reference(B, H, W, keep, scales, per_image, min_depth=1e-3):
    """grad_match_ref of make_inputs(B, H, W, keep), computed once per case."""
    pred, gt = make_inputs(B, H, W, keep)
    return grad_match_ref(pred, gt, min_depth, scales, per_image)
