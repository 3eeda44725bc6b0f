"""utils/depth_utils.py surface: cal_eval_mask and tcompute_errors with the
reference's semantics (numpy, per image), plus the GPU path the evaluation
loop uses at dataset scale: the crop is a rectangle, so `eval_crop_rect`
computes it with the reference's formulas and `tcompute_errors_gpu` reduces
the 9 metrics for a whole batch in one libmdemi launch pair
(mdemi_depth_metrics: per-image fixed-order sums, fp64 finalize).  cfg eval.align
aligns each prediction to its ground truth first (median scaling, or least-squares scale and
shift in depth or in inverse depth): on the GPU inside `tcompute_errors_gpu`
(mdemi_depth_align + mdemi_depth_metrics_aligned), on the CPU with `align_depth`.  cfg eval.tile
predicts in overlapping tiles: `tile_plan` lays them out and `merge_tiles` is the CPU counterpart
of the GPU merge (mdemi.functional.tile_merge).  cfg eval.boundary adds the scale-invariant boundary
F1 of each image (mdemi_depth_boundary; `boundary_counts` and `boundary_f1` are its numpy counterpart)."""
from collections import namedtuple

import numpy as np

__all__ = ["cal_eval_mask", "tcompute_errors", "eval_crop_rect", "tcompute_errors_gpu", "METRICS", "ALIGN_MODES",
           "check_align_mode", "align_depth", "TILE_ALIGN_MODES", "TILE_MAX_AXIS", "TilePlan", "check_tile_align",
           "tile_plan", "tile_weights", "check_tile_merge", "merge_tiles", "BOUNDARY_KEYS", "BOUNDARY_MAX_T",
           "BOUNDARY_DEFAULTS", "check_boundary", "boundary_thresholds", "boundary_counts", "boundary_f1"]

METRICS = ("a1", "a2", "a3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log_10")
ALIGN_MODES = ("none", "median", "lstsq", "lstsq_disp")
TILE_ALIGN_MODES = ("none", "lstsq", "lstsq_disp")
TILE_MAX_AXIS = 32  # MDEMI_TILE_MAX_AXIS
TilePlan = namedtuple("TilePlan", "ys xs tile overlap size")
BOUNDARY_KEYS = ("boundary_f1", "boundary_precision", "boundary_recall")
BOUNDARY_MAX_T = 16  # MDEMI_BOUNDARY_MAX_T
BOUNDARY_DEFAULTS = {"t_min": 1.05, "t_max": 1.25, "n": 10}


def check_align_mode(mode, what="eval.align"):
    if not isinstance(mode, str) or mode not in ALIGN_MODES:
        raise ValueError(f"{what} must be one of {ALIGN_MODES}, got {mode!r}")
    return mode


def eval_crop_rect(opt, gt_height, gt_width, data_type: str):
    """(y0, y1, x0, x1) of the evaluation crop (depth_utils.py:4-29)."""
    if opt["garg_crop"]:
        return (int(0.40810811 * gt_height), int(0.99189189 * gt_height),
                int(0.03594771 * gt_width), int(0.96405229 * gt_width))
    if opt["eigen_crop"]:
        if data_type in ("KITTI", "ONLINE"):
            return (int(0.3324324 * gt_height), int(0.91351351 * gt_height),
                    int(0.0359477 * gt_width), int(0.96405229 * gt_width))
        if data_type == "NYU":
            return (45, 471, 41, 601)
        raise ValueError(f"Unsupported data_type {data_type}.")
    raise ValueError("Unsupported crop configuration.")


def cal_eval_mask(opt, gt_depth, data_type: str):
    gh, gw = gt_depth.shape[-2:]
    y0, y1, x0, x1 = eval_crop_rect(opt, gh, gw, data_type)
    mask = np.zeros(gt_depth.shape[-2:], dtype=bool)
    mask[y0:y1, x0:x1] = True
    return mask


def tcompute_errors(gt: np.ndarray, pred: np.ndarray) -> dict:
    """The reference's 9 metrics on already-masked 1-D arrays (depth_utils.py:32-54)."""
    thresh = np.maximum(gt / pred, pred / gt)
    err = np.log(pred) - np.log(gt)
    return dict(a1=(thresh < 1.25).mean(), a2=(thresh < 1.25 ** 2).mean(), a3=(thresh < 1.25 ** 3).mean(),
                abs_rel=np.mean(np.abs(gt - pred) / gt), sq_rel=np.mean(((gt - pred) ** 2) / gt),
                rmse=np.sqrt(((gt - pred) ** 2).mean()),
                rmse_log=np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean()),
                silog=np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100,
                log_10=(np.abs(np.log10(gt) - np.log10(pred))).mean())


def align_depth(gt: np.ndarray, pred: np.ndarray, mode: str, max_depth: float):
    """(aligned pred, s, t) on already-masked 1-D arrays, the CPU counterpart of the GPU path
    (fp64 throughout).  "median": s = median(gt) / median(pred), t = 0; "lstsq":
    (s, t) minimise sum (s pred + t - gt)^2; "lstsq_disp": the same on 1 / pred and 1 / gt, the
    aligned depth 1 / max(s / pred + t, 1 / max_depth).  An input that cannot be aligned (no
    pixel, median(pred) not > 0, a determinant not finite and > 0) comes back as it is, with
    s = 1 and t = 0; so does mode "none".  The result is not clamped."""
    check_align_mode(mode, "mode")
    gt, pred = np.asarray(gt), np.asarray(pred)
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    n = p.size
    if mode == "none" or n == 0:
        return p, 1.0, 0.0
    with np.errstate(all="ignore"):
        if mode == "median":
            m = float(np.median(p))
            if not m > 0:
                return p, 1.0, 0.0
            s = float(np.median(g)) / m
            return s * p, s, 0.0
        x, y = (1.0 / p, 1.0 / g) if mode == "lstsq_disp" else (p, g)
        sx, sy, sxx, sxy = x.sum(), y.sum(), (x * x).sum(), (x * y).sum()
        det = n * sxx - sx * sx
        if not (np.isfinite(det) and det > 0):
            return p, 1.0, 0.0
        s, t = float((n * sxy - sx * sy) / det), float((sxx * sy - sx * sxy) / det)
        if mode == "lstsq_disp":
            return 1.0 / np.maximum(s * x + t, 1.0 / max_depth), s, t
        return s * p + t, s, t


def check_tile_align(mode, what="eval.tile_align"):
    if not isinstance(mode, str) or mode not in TILE_ALIGN_MODES:
        raise ValueError(f"{what} must be one of {TILE_ALIGN_MODES}, got {mode!r}")
    return mode


def _pair(v, what, least):
    """An int, or a list of two, >= least -> (a, b); booleans and floats are refused."""
    vs = (v, v) if isinstance(v, int) else tuple(v) if isinstance(v, (list, tuple)) else None
    if (vs is None or len(vs) != 2
            or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a < least for a in vs)):
        raise ValueError(f"{what} must be an integer >= {least} or a list of two, got {v!r}")
    return int(vs[0]), int(vs[1])


def _axis_plan(size, tile, overlap, axis):
    tile = min(tile, size)
    if not 0 <= overlap < tile:
        raise ValueError(f"tile_plan: the {axis} overlap {overlap} must be in [0, {tile}), the tile clipped to the image")
    if size == tile:
        return tile, [0]
    n = -(-(size - overlap) // (tile - overlap))
    if n > TILE_MAX_AXIS:
        raise ValueError(f"tile_plan: {n} tiles along {axis} ({size} from tiles of {tile} overlapping {overlap}); "
                         f"at most {TILE_MAX_AXIS}")
    return tile, [(i * (size - tile)) // (n - 1) for i in range(n)]


def tile_plan(H, W, tile, overlap=0):
    """The sliding-window plan of DESIGN.md §1c for an H x W image: TilePlan(ys, xs, tile, overlap,
    size), ys / xs the tiles' origins.  Per axis the tile is clipped to the image first, 0 <= overlap
    < tile is required, the tiles are n = ceil((H - o) / (t - o)) (1 when H == t) with origins
    (i (H - t)) // (n - 1): every tile inside the image, the first at 0, the last at H - t,
    neighbours overlapping by at least o.  Tile k = iy * len(xs) + ix (raster order)."""
    H, W = _pair((H, W), "tile_plan: the image size", 1)
    th, tw = _pair(tile, "tile_plan: tile", 1)
    oy, ox = _pair(overlap, "tile_plan: overlap", 0)
    th, ys = _axis_plan(H, th, oy, "y")
    tw, xs = _axis_plan(W, tw, ox, "x")
    return TilePlan(ys, xs, (th, tw), (oy, ox), (H, W))


def tile_weights(plan):
    """(wy [th], wx [tw]) fp64: the blend ramps min(u + 1, t - u, max(1, overlap)) of a tile's rows
    and columns; a pixel of a tile weighs wy[u] * wx[v]."""
    out = []
    for t, o in zip(plan.tile, plan.overlap):
        u = np.arange(t)
        out.append(np.minimum(np.minimum(u + 1, t - u), max(1, o)).astype(np.float64))
    return tuple(out)


def check_tile_merge(plan, align, max_depth):
    """The refusals tile_merge and merge_tiles share."""
    check_tile_align(align, "align")
    if align != "none":
        for n, o, axis in zip((len(plan.ys), len(plan.xs)), plan.overlap, "yx"):
            if n > 1 and o == 0:
                raise ValueError(f"align {align!r} fits each tile in its overlap with the tiles before it: the {axis} "
                                 f"axis has {n} tiles and an overlap of 0")
    if align == "lstsq_disp" and not (max_depth is not None and max_depth > 0):
        raise ValueError(f"align 'lstsq_disp' needs max_depth > 0, got {max_depth!r}")


def merge_tiles(tiles, plan, align="none", max_depth=None):
    """Per-tile predictions -> (depth (B,1,H,W) fp32, coef (B,T,4) fp64 or None): the CPU counterpart
    of mdemi.functional.tile_merge (fp64 throughout, rounded once).  tiles is
    (B*T,1,th,tw) or (B*T,th,tw), image b's tile k at b*T + k.  "none": the ramp-weighted mean of
    the covering tiles.  "lstsq" / "lstsq_disp": tile 0 anchors; each later tile k is first fitted
    (s, t) -- in depth, or in inverse depth -- to the blend of the tiles before it over the pixels
    they share, coef[b][k] = s, t, n, status; status 1 (s = 1, t = 0) marks a tile that could not
    be fitted (n < 2, a determinant not finite and > 0, s not > 0).  Under "lstsq_disp" the blend
    runs in inverse depth and the result is 1 / max(blend, 1 / max_depth)."""
    check_tile_merge(plan, align, max_depth)
    tiles = np.asarray(tiles)
    (th, tw), (H, W) = plan.tile, plan.size
    T = len(plan.ys) * len(plan.xs)
    if tiles.ndim == 4 and tiles.shape[1] == 1:
        tiles = tiles[:, 0]
    if tiles.ndim != 3 or tiles.shape[1:] != (th, tw) or tiles.shape[0] % T:
        raise ValueError(f"merge_tiles: tiles must be (B*{T},1,{th},{tw}) or (B*{T},{th},{tw}), got {tiles.shape}")
    B = tiles.shape[0] // T
    wy, wx = tile_weights(plan)
    w = wy[:, None] * wx[None, :]
    disp = align == "lstsq_disp"
    out = np.empty((B, 1, H, W), np.float32)
    coef = None if align == "none" else np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (B, T, 1))
    with np.errstate(all="ignore"):
        for b in range(B):
            num, den = np.zeros((H, W)), np.zeros((H, W))
            for k in range(T):
                y0, x0 = plan.ys[k // len(plan.xs)], plan.xs[k % len(plan.xs)]
                rect = (slice(y0, y0 + th), slice(x0, x0 + tw))
                p = tiles[b * T + k].astype(np.float64)
                x = 1.0 / p if disp else p
                s, t = 1.0, 0.0
                if align != "none" and k > 0:
                    y = num[rect] / den[rect]
                    use = (den[rect] > 0) & np.isfinite(x) & np.isfinite(y)
                    if disp:
                        use &= p > 0
                    xs_, ys_ = x[use], y[use]
                    n = xs_.size
                    sx, sy, sxx, sxy = xs_.sum(), ys_.sum(), (xs_ * xs_).sum(), (xs_ * ys_).sum()
                    det = n * sxx - sx * sx
                    ok = n >= 2 and np.isfinite(det) and det > 0
                    if ok:
                        s, t = float((n * sxy - sx * sy) / det), float((sxx * sy - sx * sxy) / det)
                        ok = s > 0
                    if not ok:
                        s, t = 1.0, 0.0
                    coef[b, k] = (s, t, n, 0.0 if ok else 1.0)
                num[rect] += w * (s * x + t if align != "none" else x)
                den[rect] += w
            r = num / den
            if disp:
                r = 1.0 / np.maximum(r, 1.0 / max_depth)
            out[b, 0] = r.astype(np.float32)
    return out, coef


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_boundary(spec, what="eval.boundary"):
    """eval.boundary, validated: None when it is absent (None) or False; True -> the defaults
    (1.05, 1.25, 10); {"t_min", "t_max", "n"} (each optional) -> (t_min, t_max, n) with
    1 < t_min <= t_max and 1 <= n <= 16.  Anything else raises a ValueError naming the key."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict):
        raise ValueError(f"{what} must be true, false or an object with t_min / t_max / n, got {spec!r}")
    unknown = [k for k in spec if k not in BOUNDARY_DEFAULTS]
    if unknown:
        raise ValueError(f"{what}.{unknown[0]} is not a key of {what}: it takes {tuple(BOUNDARY_DEFAULTS)}")
    v = {**BOUNDARY_DEFAULTS, **spec}
    t_min, t_max, n = v["t_min"], v["t_max"], v["n"]
    if not (_number(t_min) and np.isfinite(t_min) and t_min > 1):
        raise ValueError(f"{what}.t_min must be a number above 1, got {t_min!r}")
    if not (_number(t_max) and np.isfinite(t_max) and t_max >= t_min):
        raise ValueError(f"{what}.t_max must be a number not below t_min = {t_min!r}, got {t_max!r}")
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= n <= BOUNDARY_MAX_T:
        raise ValueError(f"{what}.n must be an integer in 1..{BOUNDARY_MAX_T}, got {n!r}")
    return float(t_min), float(t_max), int(n)


def boundary_thresholds(t_min=1.05, t_max=1.25, n=10):
    """The n thresholds of DESIGN.md §1c: np.linspace(t_min, t_max, n) rounded to fp32."""
    t_min, t_max, n = check_boundary({"t_min": t_min, "t_max": t_max, "n": n}, "boundary_thresholds")
    t = np.linspace(t_min, t_max, n).astype(np.float32)
    if not (t[0] > 1 and np.all(np.diff(t) >= 0)):
        raise ValueError(f"boundary_thresholds: t_min = {t_min!r} rounds to 1 in fp32")
    return t


def _thresholds32(thresholds):
    t = np.asarray(thresholds)
    if t.dtype != np.float32 or t.ndim != 1 or not 1 <= t.size <= BOUNDARY_MAX_T:
        raise ValueError(f"thresholds must be 1..{BOUNDARY_MAX_T} float32 values (boundary_thresholds), got {t!r}")
    if not (np.all(np.isfinite(t)) and t[0] > 1 and np.all(np.diff(t) >= 0)):
        raise ValueError(f"thresholds must be finite, above 1 and non-decreasing, got {t!r}")
    return t


def boundary_counts(gt, pred, valid, thresholds):
    """The edge counts of DESIGN.md §1c on 2-D maps, the CPU counterpart of mdemi_depth_boundary:
    (n, 4, 3) int64 = per threshold and kind (right, left, lower, upper is farther) the pairs of
    adjacent valid pixels that are an edge in gt, in pred and in both.  pred is the evaluated value
    (aligned and clamped already); every compare is fp32: b > fl32(tau a)."""
    t = _thresholds32(thresholds)
    g, q, v = np.asarray(gt, np.float32), np.asarray(pred, np.float32), np.asarray(valid, bool)
    if g.ndim != 2 or q.shape != g.shape or v.shape != g.shape:
        raise ValueError(f"boundary_counts: gt, pred and valid must be 2-D maps of one shape, got {g.shape}, "
                         f"{q.shape}, {v.shape}")
    out = np.zeros((t.size, 4, 3), np.int64)
    with np.errstate(all="ignore"):
        for d, (a, b) in enumerate(((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :]))):
            both = v[a] & v[b]
            for i, tau in enumerate(t):
                for k, (lo, hi) in enumerate(((a, b), (b, a))):
                    eg = both & (g[hi] > tau * g[lo])
                    eq = both & (q[hi] > tau * q[lo])
                    out[i, 2 * d + k] = eg.sum(), eq.sum(), (eg & eq).sum()
    return out


def boundary_f1(counts, thresholds):
    """Counts (n, 4, 3) -> {"boundary_f1", "boundary_precision", "boundary_recall"} in fp64, or None
    for an image whose ground truth has no edge at the lowest threshold: per
    threshold P = mean over the kinds of tp / max(pred, 1), R the same over gt, F their harmonic
    mean (0 when both are 0); the scores are the means over the thresholds weighted by tau."""
    t = _thresholds32(thresholds).astype(np.float64)
    c = np.asarray(counts)
    if c.shape != (t.size, 4, 3):
        raise ValueError(f"boundary_f1: counts must be ({t.size}, 4, 3), got {c.shape}")
    if int(c[0, :, 0].sum()) == 0:
        return None
    tsum = 0.0
    for tau in t:
        tsum += float(tau)
    f1 = prec = rec = 0.0
    for i in range(t.size):
        p = r = 0.0
        for k in range(4):
            n_gt, n_pr, n_tp = (int(x) for x in c[i, k])
            p += n_tp / max(n_pr, 1)
            r += n_tp / max(n_gt, 1)
        p *= 0.25
        r *= 0.25
        f = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
        w = float(t[i]) / tsum
        f1 += w * f
        prec += w * p
        rec += w * r
    return dict(zip(BOUNDARY_KEYS, (f1, prec, rec)))


def tcompute_errors_gpu(pred, gt, eval_opt, data_type, clamp_pred=True):
    """Per-image metrics for a batch on the GPU: pred/gt (B, 1, H, W) fp32 CUDA tensors; valid =
    crop & min_depth_eval < gt < max_depth_eval (cfg eval.*).  Returns a list of dicts (one per
    image, the reference's keys) -- feed them to RunningAverageDict / all_reduce_dict.  With
    eval.align other than "none" they are the metrics of the per-image aligned prediction.  With
    eval.boundary each dict also carries BOUNDARY_KEYS, the boundary scores of the same evaluated
    value -- except for an image that has no score (no ground-truth edge), which carries none."""
    from .. import functional as mf
    h, w = gt.shape[-2:]
    rect = eval_crop_rect(eval_opt, h, w, data_type)
    align = check_align_mode(eval_opt.get("align", "none"))
    boundary = check_boundary(eval_opt.get("boundary"))
    align = None if align == "none" else align
    dmin, dmax = eval_opt["min_depth_eval"], eval_opt["max_depth_eval"]
    if boundary is None:
        out = mf.depth_metrics(pred, gt, rect, dmin, dmax, clamp_pred=clamp_pred, align=align)
        return [dict(zip(METRICS, row[:9].tolist())) for row in out.cpu().numpy()]
    # one alignment serves both: the metrics and the edges are those of the same q
    coef = None if align is None else mf.depth_align(pred, gt, rect, dmin, dmax, align)
    out = mf.depth_metrics(pred, gt, rect, dmin, dmax, clamp_pred=clamp_pred, align=align, coef=coef)
    edge = mf.depth_boundary(pred, gt, rect, dmin, dmax, clamp_pred=clamp_pred, align=align, coef=coef,
                             thresholds=boundary_thresholds(*boundary)).cpu().numpy()
    rows = [dict(zip(METRICS, row[:9].tolist())) for row in out.cpu().numpy()]
    for row, e in zip(rows, edge):
        if e[4] == 0:
            row.update(zip(BOUNDARY_KEYS, e[:3].tolist()))
    return rows
