"""Plain-numpy fp64 reference of the per-image depth alignment (cfg eval.align)
and the seeded inputs the GPU tests share.

Per image, V = crop rectangle & min_depth < gt < max_depth, p the unclamped prediction and g the
ground truth on V, n = |V|:
  median      s = median(g) / median(p), t = 0; the order statistics on the fp32 values, for even n
              the mean of the two middle ones, mean and quotient in fp64
  lstsq       det = n Spp - Sp^2, s = (n Spg - Sp Sg) / det, t = (Spp Sg - Sp Spg) / det, fp64 sums
  lstsq_disp  the same on x = 1/p, y = 1/g; aligned depth 1 / max(s/p + t, 1/max_depth)
q = (float)(s p + t) (or the lstsq_disp form), formed in fp64 and rounded once, then clamped into
[min_depth, max_depth] for the nine metrics.  An image with n == 0, median(p) not > 0 or det not
finite and > 0 is evaluated unaligned: s = 1, t = 0, status 1, q = p."""
import functools

import numpy as np

MODES = ("median", "lstsq", "lstsq_disp")
DMIN, DMAX = 1e-3, 80.0
METRICS = ("a1", "a2", "a3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log_10")

# (B, H, W, keep, seed): one chunk with an odd W; KITTI-sparse over several chunks (9170 pixels).
# With seed 0 the preconditions below hold in every mode; n is 747 / 750 / 765 and 365 / 366.
SHAPES = [(3, 37, 53, 0.6, 0), (2, 70, 131, 0.05, 0)]


def rect_of(H, W):
    return (5, H - 3, 4, W - 6)


def valid_mask(gt, rect, dmin=DMIN, dmax=DMAX):
    y0, y1, x0, x1 = rect
    m = np.zeros(gt.shape, bool)
    m[..., y0:y1, x0:x1] = True
    return m & (gt > np.float32(dmin)) & (gt < np.float32(dmax))


def solve(p32, g32, mode):
    """(s, t, status) of one image from its fp32 valid pixels."""
    n = p32.size
    if n == 0:
        return 1.0, 0.0, 1
    p, g = p32.astype(np.float64), g32.astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == "median":
            sp, sg = np.sort(p), np.sort(g)
            lo, hi = (n - 1) // 2, n // 2
            mp, mg = 0.5 * (sp[lo] + sp[hi]), 0.5 * (sg[lo] + sg[hi])
            return (mg / mp, 0.0, 0) if mp > 0 else (1.0, 0.0, 1)
        x, y = (1.0 / p, 1.0 / g) if mode == "lstsq_disp" else (p, g)
        sx, sy, sxx, sxy = x.sum(), y.sum(), (x * x).sum(), (x * y).sum()
        det = n * sxx - sx * sx
        if not (np.isfinite(det) and det > 0):
            return 1.0, 0.0, 1
        return (n * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det, 0


def aligned_value(pred32, s, t, status, mode, dmax=DMAX):
    """q before the clamp, fp32, on every pixel of one image."""
    if status:
        return pred32.copy()
    p = pred32.astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == "lstsq_disp":
            return (1.0 / np.maximum(s / p + t, 1.0 / np.float64(np.float32(dmax)))).astype(np.float32)
        return (s * p + t).astype(np.float32)


def metrics_of(g, q):
    """The nine metrics in fp64 on masked arrays (tcompute_errors' formulas)."""
    g, q = g.astype(np.float64), q.astype(np.float64)
    th = np.maximum(g / q, q / g)
    err = np.log(q) - np.log(g)
    return np.array([(th < 1.25).mean(), (th < 1.25 ** 2).mean(), (th < 1.25 ** 3).mean(),
                     np.mean(np.abs(g - q) / g), np.mean((g - q) ** 2 / g), np.sqrt(((g - q) ** 2).mean()),
                     np.sqrt((err ** 2).mean()), np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100,
                     np.abs(np.log10(g) - np.log10(q)).mean()])


def align_ref(pred, gt, rect, mode, dmin=DMIN, dmax=DMAX):
    """pred, gt (B, H, W) fp32 -> dict(coef (B, 4) = s, t, n, status; q (B, H, W) fp32 before the
    clamp; metrics (B, 9) fp64 of the clamped q; mask (B, H, W))."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    mask = valid_mask(gt, rect, dmin, dmax)
    B = pred.shape[0]
    coef, q, met = np.zeros((B, 4)), np.empty_like(pred), np.zeros((B, 9))
    for b in range(B):
        m = mask[b]
        s, t, status = solve(pred[b][m], gt[b][m], mode)
        coef[b] = s, t, m.sum(), status
        q[b] = aligned_value(pred[b], s, t, status, mode, dmax)
        if m.any():
            met[b] = metrics_of(gt[b][m], np.clip(q[b][m], np.float32(dmin), np.float32(dmax)))
    return dict(coef=coef, q=q, metrics=met, mask=mask)


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, keep, seed):
    """(pred, gt) float32 (B, H, W): gt = exp(U(log 0.5, log 60)), zeroed where a uniform draw
    exceeds keep; pred = (0.37 gt + 1.9) exp(0.1 N(0, 1)) of the unzeroed gt."""
    rng = np.random.default_rng(seed)
    gt = np.exp(rng.uniform(np.log(0.5), np.log(60.0), (B, H, W)))
    pred = (0.37 * gt + 1.9) * np.exp(0.1 * rng.standard_normal((B, H, W)))
    drop = rng.uniform(size=(B, H, W)) > keep
    pred, gt = pred.astype(np.float32), gt.astype(np.float32)
    gt[drop] = 0.0
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


def check_preconditions(shapes=SHAPES, rect=None):
    """What the GPU tests lean on, asserted on the CPU (rect: another rectangle than rect_of's):
    both parities of n occur; x varies enough that the det cancellation amplifies a
    summation-order difference by no more than ~12 (cv >= 0.3); no valid pixel's threshold ratio
    sits within 1e-5 relative of a delta cut, where a 1-ulp difference in q could move a pixel
    across it."""
    parities = set()
    for (B, H, W, keep, seed) in shapes:
        pred, gt = make_inputs(B, H, W, keep, seed)
        for mode in MODES:
            r = reference(B, H, W, keep, seed, mode, rect)
            assert not r["coef"][:, 3].any(), (B, H, W, mode, "an image failed to align")
            for b in range(B):
                m = r["mask"][b]
                parities.add(int(m.sum()) % 2)
                if mode != "median":
                    x = pred[b][m].astype(np.float64)
                    x = 1.0 / x if mode == "lstsq_disp" else x
                    assert x.std() / abs(x.mean()) >= 0.3, (B, H, W, mode, b, "cv")
                g = gt[b][m].astype(np.float64)
                q = np.clip(r["q"][b][m], np.float32(DMIN), np.float32(DMAX)).astype(np.float64)
                th = np.maximum(g / q, q / g)
                for cut in (1.25, 1.25 ** 2, 1.25 ** 3):
                    assert np.abs(th / cut - 1.0).min() > 1e-5, (B, H, W, mode, b, cut, "threshold tie")
    assert rect is not None or parities == {0, 1}, parities  # of the tests' own rectangle


@functools.lru_cache(maxsize=None)
def reference(B, H, W, keep, seed, mode, rect=None):
    """align_ref of make_inputs(B, H, W, keep, seed), computed once per case."""
    pred, gt = make_inputs(B, H, W, keep, seed)
    return align_ref(pred, gt, rect_of(H, W) if rect is None else rect, mode)


def ulp_diff64(a, b):
    """|a - b| in units of fp64 ulps (finite values of one sign)."""
    ia = np.asarray(a, np.float64).view(np.int64)
    ib = np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def ulp_diff32(a, b):
    """|a - b| in fp32 ulps, through the monotone integer image of the float bits."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
