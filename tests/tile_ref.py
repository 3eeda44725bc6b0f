"""An fp64 numpy statement of tiled inference's merge, independent of the package:
the plan, the ramp weights, the sequential per-tile alignment and the blend, written as plain
loops over tiles.  Every tile's target is gathered from the tiles before it, as the kernels do;
nothing is shared with mdemi.utils.depth_utils.merge_tiles."""
import numpy as np


def axis_origins(size, tile, overlap):
    """(clipped tile, origins) along one axis."""
    tile = min(tile, size)
    assert 0 <= overlap < tile
    if size == tile:
        return tile, [0]
    n = (size - overlap + (tile - overlap) - 1) // (tile - overlap)
    return tile, [(i * (size - tile)) // (n - 1) for i in range(n)]


def ramp(t, overlap):
    return np.array([min(u + 1, t - u, max(1, overlap)) for u in range(t)], dtype=np.float64)


def _q(p, s, t, align):
    p = p.astype(np.float64)
    if align == "none":
        return p
    return s * (1.0 / p if align == "lstsq_disp" else p) + t


def _blend_onto(rect, tiles, coef, boxes, w, upto, align):
    """num, den over the rectangle rect = (y0, y1, x0, x1) of the tiles k < upto, in ascending k."""
    y0, y1, x0, x1 = rect
    num, den = np.zeros((y1 - y0, x1 - x0)), np.zeros((y1 - y0, x1 - x0))
    for k in range(upto):
        ty, tx = boxes[k]
        th, tw = w.shape
        a0, a1, b0, b1 = max(y0, ty), min(y1, ty + th), max(x0, tx), min(x1, tx + tw)
        if a0 >= a1 or b0 >= b1:
            continue
        wk = w[a0 - ty:a1 - ty, b0 - tx:b1 - tx]
        qk = _q(tiles[k][a0 - ty:a1 - ty, b0 - tx:b1 - tx], coef[k][0], coef[k][1], align)
        num[a0 - y0:a1 - y0, b0 - x0:b1 - x0] += wk * qk
        den[a0 - y0:a1 - y0, b0 - x0:b1 - x0] += wk
    return num, den


def fit(x, y):
    """(s, t, n, status) of argmin sum (s x + t - y)^2 with the failure rule."""
    n = x.size
    sx, sy, sxx, sxy = x.sum(), y.sum(), (x * x).sum(), (x * y).sum()
    det = n * sxx - sx * sx
    if n < 2 or not np.isfinite(det) or not det > 0:
        return 1.0, 0.0, float(n), 1.0
    s, t = (n * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det
    if not s > 0:
        return 1.0, 0.0, float(n), 1.0
    return float(s), float(t), float(n), 0.0


def merge(tiles, size, tile, overlap, align="none", max_depth=None, diag=None):
    """tiles (B*T, th, tw) fp32 -> (out (B, H, W) fp32, coef (B, T, 4) fp64, blend (B, H, W) fp64: out
    before its rounding).  diag: a list that receives, per fit, (b, k, the coefficient of variation
    of x, mean |y|)."""
    (H, W), (oy, ox) = size, overlap
    th, ys = axis_origins(H, tile[0], oy)
    tw, xs = axis_origins(W, tile[1], ox)
    boxes = [(y, x) for y in ys for x in xs]
    T = len(boxes)
    assert tiles.shape[1:] == (th, tw) and tiles.shape[0] % T == 0
    B = tiles.shape[0] // T
    w = ramp(th, oy)[:, None] * ramp(tw, ox)[None, :]
    out, out64, coefs = np.empty((B, H, W), np.float32), np.empty((B, H, W)), np.zeros((B, T, 4))
    with np.errstate(all="ignore"):
        for b in range(B):
            mine = tiles[b * T:(b + 1) * T]
            coef = [(1.0, 0.0, 0.0, 0.0)] * T
            if align != "none":
                for k in range(1, T):
                    ty, tx = boxes[k]
                    num, den = _blend_onto((ty, ty + th, tx, tx + tw), mine, coef, boxes, w, k, align)
                    p = mine[k].astype(np.float64)
                    x = 1.0 / p if align == "lstsq_disp" else p
                    y = num / den
                    use = (den > 0) & np.isfinite(x) & np.isfinite(y)
                    if align == "lstsq_disp":
                        use &= p > 0
                    coef[k] = fit(x[use], y[use])
                    if diag is not None and use.any():
                        diag.append((b, k, x[use].std() / abs(x[use].mean()), np.abs(y[use]).mean()))
            num, den = _blend_onto((0, H, 0, W), mine, coef, boxes, w, T, align)
            r = num / den
            if align == "lstsq_disp":
                r = 1.0 / np.maximum(r, 1.0 / max_depth)
            out64[b], out[b], coefs[b] = r, r.astype(np.float32), np.array(coef)
    return out, coefs, out64


def cut(maps, size, tile, overlap):
    """maps (B, H, W) -> its tiles (B*T, th, tw), image b's tile k at b*T + k."""
    th, ys = axis_origins(size[0], tile[0], overlap[0])
    tw, xs = axis_origins(size[1], tile[1], overlap[1])
    return np.stack([m[y:y + th, x:x + tw] for m in maps for y in ys for x in xs])


DEPTH_RANGE = (1.0, 9.0)
MAX_DEPTH = 10.0


def recoverable(size, tile, overlap, align, B=2, seed=0, noise=0.0):
    """(D (B, H, W) fp64, tiles (B*T, th, tw) fp32): tiles cut from the map D, then tile k > 0 of every
    image given its own transform, s in [0.5, 2] and t within +-10 % of the range of D (of 1 / D for
    "lstsq_disp"), so that s p_k + t (s / p_k + t) is D (1 / D) on the tile; tile 0 keeps D's frame.
    noise: relative, uniform in +-noise, on every tile value."""
    rng = np.random.default_rng(seed)
    H, W = size
    yy, xx = np.mgrid[0:H, 0:W]
    lo, hi = DEPTH_RANGE
    D = np.stack([lo + (hi - lo) * (0.5 + 0.1 * np.sin(0.23 * yy + 0.7 * b) * np.cos(0.17 * xx + b)
                                    + 0.4 * rng.uniform(-1, 1, size=(H, W))) for b in range(B)])
    assert D.min() >= lo and D.max() <= hi
    disp = align == "lstsq_disp"
    target = cut(1.0 / D if disp else D, size, tile, overlap)
    T = target.shape[0] // B
    span = (1.0 / lo - 1.0 / hi) if disp else (hi - lo)
    s = rng.uniform(0.5, 2.0, size=B * T)
    t = rng.uniform(-0.1, 0.1, size=B * T) * span
    s[::T], t[::T] = 1.0, 0.0
    x = (target - t[:, None, None]) / s[:, None, None]
    assert x.min() > 0
    p = 1.0 / x if disp else x
    p = p * (1.0 + noise * rng.uniform(-1, 1, size=p.shape))
    return D, p.astype(np.float32)


def ulp_diff(a, b):
    """|a - b| in fp32 units in the last place (of b's binade); 0 where both are NaN or equal."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
    d = np.where(both_nan | (a == b), 0.0, d)
    return np.where(np.isnan(d), np.inf, d)
