"""Plain-numpy reference of the scale-invariant boundary F1 (cfg eval.boundary) and
the seeded inputs the GPU tests share.  Independent of mdemi.utils.depth_utils: one slice per
direction and one compare per threshold, as the definition reads.

Per image, g the ground truth, q the evaluated prediction (aligned, clamped), V = crop rectangle &
dmin < g < dmax.  A pair is two horizontally or vertically adjacent pixels both in V.  At threshold
tau_i = float32(linspace(t_min, t_max, n))[i] a pair (a, b) -- b the right or the lower neighbour --
of a map d is an edge of kind
  0 / 2  right / lower is farther   d[b] > fl32(tau_i d[a])
  1 / 3  left / upper is farther    d[a] > fl32(tau_i d[b])
counts[i][k] = (edges of g, edges of q, edges of both).  In fp64: P_i = mean_k tp / max(pred, 1),
R_i = mean_k tp / max(gt, 1), F_i = 2 P_i R_i / (P_i + R_i) (0 when both are 0), w_i = tau_i / sum tau;
f1, precision, recall = sum w_i F_i, sum w_i P_i, sum w_i R_i.  An image whose ground truth has no
edge at tau_0 has no score: status 1, scores 0."""
import functools

import numpy as np

DMIN, DMAX = 1e-3, 10.0
T_MIN, T_MAX, N_T = 1.05, 1.25, 10

# (B, H, W, seed): odd width (scalar path); W % 4 == 0 (vector path); one pair direction only,
# twice; more rows than one workgroup takes at this width (at least three row chunks).  The seeds
# are those at which check_preconditions holds; precision and recall come out in 0.53 .. 0.78.
SHAPES = [(3, 37, 53, 1), (2, 48, 64, 2), (1, 1, 9, 1), (1, 9, 1, 0), (2, 300, 68, 0)]


def thresholds(t_min=T_MIN, t_max=T_MAX, n=N_T):
    return np.linspace(t_min, t_max, n).astype(np.float32)


def rect_of(H, W):
    """An interior crop; the whole image where it is too small to have an interior."""
    return (5, H - 3, 4, W - 6) if H >= 12 and W >= 12 else (0, H, 0, W)


def valid_mask(gt, rect, dmin=DMIN, dmax=DMAX):
    y0, y1, x0, x1 = rect
    m = np.zeros(gt.shape, bool)
    m[..., y0:y1, x0:x1] = True
    return m & (gt > np.float32(dmin)) & (gt < np.float32(dmax))


def evaluated(pred, clamp=True, dmin=DMIN, dmax=DMAX):
    """q of an unaligned prediction: the clamp into [dmin, dmax], in fp32."""
    pred = np.asarray(pred, np.float32)
    return np.clip(pred, np.float32(dmin), np.float32(dmax)) if clamp else pred


def counts_of(g, q, valid, thr):
    """(n, 4, 3) int64 of one image."""
    out = np.zeros((len(thr), 4, 3), np.int64)
    pairs = 0
    for d in range(2):
        if d == 0:
            first, second = (slice(None), slice(0, -1)), (slice(None), slice(1, None))
        else:
            first, second = (slice(0, -1), slice(None)), (slice(1, None), slice(None))
        ok = valid[first] & valid[second]
        pairs += int(ok.sum())
        ga, gb, qa, qb = g[first], g[second], q[first], q[second]
        for i, tau in enumerate(thr):
            tau = np.float32(tau)
            g_far_b, g_far_a = ok & (gb > tau * ga), ok & (ga > tau * gb)
            q_far_b, q_far_a = ok & (qb > tau * qa), ok & (qa > tau * qb)
            out[i, 2 * d] = g_far_b.sum(), q_far_b.sum(), (g_far_b & q_far_b).sum()
            out[i, 2 * d + 1] = g_far_a.sum(), q_far_a.sum(), (g_far_a & q_far_a).sum()
    return out, pairs


def scores_of(counts, thr):
    """(f1, precision, recall, status) in fp64."""
    t = np.asarray(thr, np.float32).astype(np.float64)
    c = counts.astype(np.float64)
    if counts[0, :, 0].sum() == 0:
        return 0.0, 0.0, 0.0, 1
    P = 0.25 * (c[:, :, 2] / np.maximum(c[:, :, 1], 1.0)).sum(axis=1)
    R = 0.25 * (c[:, :, 2] / np.maximum(c[:, :, 0], 1.0)).sum(axis=1)
    with np.errstate(all="ignore"):
        F = np.where(P + R > 0, 2.0 * P * R / (P + R), 0.0)
    w = t / t.sum()
    return float((w * F).sum()), float((w * P).sum()), float((w * R).sum()), 0


def boundary_ref(q, gt, rect, thr=None, dmin=DMIN, dmax=DMAX):
    """q (the evaluated prediction), gt (B, H, W) fp32 -> dict(counts (B, n, 4, 3) int64,
    out (B, 5) fp64 = f1, precision, recall, n_pairs, status; mask (B, H, W))."""
    thr = thresholds() if thr is None else np.asarray(thr, np.float32)
    q, gt = np.asarray(q, np.float32), np.asarray(gt, np.float32)
    assert q.dtype == np.float32 and gt.dtype == np.float32 and q.shape == gt.shape and q.ndim == 3
    mask = valid_mask(gt, rect, dmin, dmax)
    B = q.shape[0]
    counts, out = np.zeros((B, len(thr), 4, 3), np.int64), np.zeros((B, 5))
    for b in range(B):
        counts[b], pairs = counts_of(gt[b], q[b], mask[b], thr)
        out[b] = (*scores_of(counts[b], thr)[:3], pairs, scores_of(counts[b], thr)[3])
    return dict(counts=counts, out=out, mask=mask)


def _scene(rng, H, W):
    """A slanted plane with six rectangles of other depths in 1..9 m."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = 2.5 + 2.0 * yy / max(H - 1, 1) + 1.5 * xx / max(W - 1, 1)
    for _ in range(6):
        h, w = int(rng.integers(max(2, H // 6), max(3, H // 2))), int(rng.integers(max(2, W // 6), max(3, W // 2)))
        y, x = int(rng.integers(0, max(1, H - h))), int(rng.integers(0, max(1, W - w)))
        d[y:y + h, x:x + w] = rng.uniform(1.0, 9.0)
    return d


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, seed):
    """(pred, gt) float32 (B, H, W), read-only.  gt: _scene, then about 10 % holes (0) and 2 % of
    the pixels beyond DMAX.  pred: the scene before the holes, shifted one pixel in x on the lower
    half, box-blurred (3 taps) in x on the upper third, times 1 + 0.02 N(0, 1)."""
    rng = np.random.default_rng([seed, B, H, W])
    gt, pred = np.empty((B, H, W)), np.empty((B, H, W))
    for b in range(B):
        d = _scene(rng, H, W)
        p = d.copy()
        lower, upper = H // 2, (H + 2) // 3
        p[lower:] = np.roll(d[lower:], 1, axis=1)
        pad = np.pad(d[:upper], ((0, 0), (1, 1)), mode="edge")
        if H >= 3:
            p[:upper] = (pad[:, :-2] + pad[:, 1:-1] + pad[:, 2:]) / 3.0
        pred[b] = p * (1.0 + 0.02 * rng.standard_normal((H, W)))
        u = rng.uniform(size=(H, W))
        g = d.copy()
        g[u < 0.10] = 0.0
        g[u > 0.98] = rng.uniform(11.0, 15.0)
        gt[b] = g
    pred, gt = pred.astype(np.float32), gt.astype(np.float32)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def reference(B, H, W, seed, clamp=True, rect=None):
    """boundary_ref of make_inputs(B, H, W, seed), computed once per case."""
    pred, gt = make_inputs(B, H, W, seed)
    return boundary_ref(evaluated(pred, clamp), gt, rect_of(H, W) if rect is None else rect)


def check_preconditions(shapes=SHAPES):
    """What the GPU tests lean on, asserted on the CPU.  Where both pair directions exist, every
    image has, at the first and at the last threshold and in every kind, ground-truth edges, false
    positives and misses (n_gt, n_pr - n_tp and n_gt - n_tp all > 0): a kernel that drops a kind,
    a direction or a threshold cannot pass.  A one-row or one-column image has scored edges in its
    two kinds and none in the other two."""
    for (B, H, W, seed) in shapes:
        r = reference(B, H, W, seed)
        c = r["counts"]
        assert not r["out"][:, 4].any(), (B, H, W, "an image has no score")
        if H > 1 and W > 1:
            for i in (0, c.shape[1] - 1):
                n_gt, n_pr, n_tp = c[:, i, :, 0], c[:, i, :, 1], c[:, i, :, 2]
                assert (n_gt > 0).all() and (n_pr - n_tp > 0).all() and (n_gt - n_tp > 0).all(), (B, H, W, i, c[:, i])
            p, rc = r["out"][:, 1], r["out"][:, 2]
            assert (p > 0.2).all() and (p < 0.9).all() and (rc > 0.2).all() and (rc < 0.9).all(), (B, H, W, p, rc)
        else:
            here, absent = ((0, 1), (2, 3)) if H == 1 else ((2, 3), (0, 1))
            assert c[:, 0, here, 0].sum() > 0 and c[:, 0, here, 1].sum() > 0, (B, H, W, c[:, 0])
            assert c[:, :, absent, :].sum() == 0, (B, H, W)
