"""Plain-numpy fp64 reference of the scale- and shift-invariant loss (loss.ssi_weight, DESIGN.md
§1c) and the seeded inputs the GPU tests share.

Per image, on V = gt > min_depth (n pixels): x, y = pred, gt ("depth") or 1/pred, 1/gt ("disp");
(s, t) minimise sum (s x + t - y)^2 from the fp64 sums Sx, Sy, Sxx, Sxy, Syy:
det = n Sxx - Sx^2, s = (n Sxy - Sx Sy) / det, t = (Sxx Sy - Sx Sxy) / det.  r = s x + t - y,
rho = |float32(r)|.  Trimming: u = n - floor(float32(trim) n), tau = the u-th smallest rho,
K = {rho <= tau} (ties kept), U = |K|, Q = sum_K r^2, A = sum_K r x, Bt = sum_K r; trim == 0 has
K = V and A = Bt = 0 by definition.  norm "gt_var" divides by v = Syy / n - (Sy / n)^2.  An image
is skipped (loss 0, gradient exactly 0, out of the per-image mean) when n == 0, det is finite and
<= 0, or v is finite and <= 0; a non-finite det gives a NaN loss.
Per batch L = sum_b (Q_b / v_b) / (2 sum_b U_b), w_b = 1 / (v_b sum U); per image L = the mean over
the images used of Q_b / (2 U_b v_b), w_b = 1 / (U_b v_b images used).
dL/dx_i = w_b [k_i r_i s + (A - Bt Sx / n)(n y_i - Sy - 2 s (n x_i - Sx)) / det - Bt s / n];
dL/dpred = dL/dx (depth), dL/dx (-1 / pred^2) (disp); exactly 0 off V."""
import functools

import numpy as np

from grad_match_ref import SHAPES as _GM_SHAPES
from grad_match_ref import make_inputs  # noqa: F401  (the tests take the inputs from here)

NEAR = 1e-5  # a pixel with |rho - tau| <= NEAR * tau may change sides under a last-bit change of (s, t)
SHAPES = list(_GM_SHAPES) + [(2, 40, 260, 0.9)]
SPACES = ("depth", "disp")
NORMS = ("none", "gt_var")


def ssi_image(pred, gt, min_depth=1e-3, space="depth", trim=0.0, norm="none"):
    """One image (any shape).  A dict of the definition's per-image quantities; x, y, r, rho, k
    are arrays over V in raster order."""
    assert space in SPACES and norm in NORMS
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    V = gt > np.float32(min_depth)
    p, g = pred[V].astype(np.float64), gt[V].astype(np.float64)
    n = int(V.sum())
    with np.errstate(all="ignore"):
        x, y = (1.0 / p, 1.0 / g) if space == "disp" else (p, g)
        Sx, Sy, Sxx, Sxy, Syy = x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()
        det = n * Sxx - Sx * Sx
        v = (Syy / n - (Sy / n) ** 2) if (norm == "gt_var" and n > 0) else 1.0
    out = dict(V=V, n=n, Sx=Sx, Sy=Sy, det=det, v=v, x=x, y=y)
    out["skip"] = bool(n == 0 or (np.isfinite(det) and det <= 0) or (np.isfinite(v) and v <= 0))
    out["nan"] = bool(not out["skip"] and not np.isfinite(det))
    if out["skip"] or out["nan"]:
        return out
    s = (n * Sxy - Sx * Sy) / det
    t = (Sxx * Sy - Sx * Sxy) / det
    r = s * x + t - y
    with np.errstate(over="ignore"):
        rho = np.abs(r.astype(np.float32))
    near = np.zeros(n, bool)
    if trim > 0:
        u = n - int(np.floor(float(np.float32(trim)) * n))
        tau = np.partition(rho, u - 1)[u - 1]
        k = rho <= tau
        near = np.abs(rho.astype(np.float64) - float(tau)) <= NEAR * float(tau)
        if near.sum() == 1:  # the tau pixel alone: nothing can change sides
            near[:] = False
        A, Bt = (r * x)[k].sum(), r[k].sum()
    else:
        u, tau, k, A, Bt = n, np.float32(np.inf), np.ones(n, bool), 0.0, 0.0
    out.update(s=s, t=t, r=r, rho=rho, u=u, tau=tau, k=k, U=int(k.sum()), Q=(r * r)[k].sum(), A=A, Bt=Bt, near=near)
    return out


def ssi_ref(pred, gt, min_depth=1e-3, space="depth", trim=0.0, norm="none", per_image=False):
    """pred, gt (B, H, W) float32 -> (loss, dloss/dpred (B, H, W) fp64, near mask (B, H, W))."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    assert pred.ndim == 3 and pred.shape == gt.shape and 0.0 <= trim <= 0.5
    B = pred.shape[0]
    im = [ssi_image(pred[b], gt[b], min_depth, space, trim, norm) for b in range(B)]
    grad, near = np.zeros(pred.shape, np.float64), np.zeros(pred.shape, bool)
    if any(m["nan"] for m in im):  # the loss is NaN; only that much is pinned, and NaN on the image's V
        for b, m in enumerate(im):
            if m["nan"]:
                grad[b][m["V"]] = np.nan
        return float("nan"), grad, near
    used = [b for b in range(B) if not im[b]["skip"]]
    if not used:
        return 0.0, grad, near
    if per_image:
        loss = float(np.mean([im[b]["Q"] / (2.0 * im[b]["U"] * im[b]["v"]) for b in used]))
    else:
        sum_u = float(sum(im[b]["U"] for b in used))
        loss = float(sum(im[b]["Q"] / im[b]["v"] for b in used) / (2.0 * sum_u))
    for b in used:
        m = im[b]
        w = 1.0 / (m["U"] * m["v"] * len(used)) if per_image else 1.0 / (m["v"] * sum_u)
        n, x, y, s = m["n"], m["x"], m["y"], m["s"]
        d = m["k"] * m["r"] * s
        if trim > 0:
            d = d + (m["A"] - m["Bt"] * m["Sx"] / n) * (n * y - m["Sy"] - 2.0 * s * (n * x - m["Sx"])) / m["det"] \
                - m["Bt"] * s / n
        d = w * d
        if space == "disp":
            d = d * (-(x * x))  # dx/dpred = -1 / pred^2
        grad[b][m["V"]] = d
        near[b][m["V"]] = m["near"]
    return loss, grad, near


@functools.lru_cache(maxsize=None)
def reference(B, H, W, keep, space, trim, norm, per_image, min_depth=1e-3):
    """ssi_ref of make_inputs(B, H, W, keep), computed once per case."""
    pred, gt = make_inputs(B, H, W, keep)
    return ssi_ref(pred, gt, min_depth, space, trim, norm, per_image)
