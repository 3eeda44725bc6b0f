"""Evaluation path on the GPU: inference, flip-eval, the
9 depth metrics and their cross-rank mean.

The reference's driver (run.py) is absent from the snapshot; what it did is
fixed by the config keys eval.{min_depth_eval, max_depth_eval, garg_crop,
eigen_crop, flip_eval} (json/{nyu,kitti}/*.json) and by the helpers it
called: cal_eval_mask + tcompute_errors (utils/depth_utils.py:4-54),
RunningAverageDict (utils/common_utils.py:92-135) and
all_reduce_dict(op="mean") (utils/dist_utils.py:67-76).  Restated here (parity
of the driver itself is unpinned; each helper is pinned by its own tests):

  pred = model(img)                       # depth, NCHW
  if flip_eval: pred = (pred + flip_w(model(flip_w(img)))) / 2
  pred -> GT resolution (bilinear, align_corners=True) when the model
          predicts at half resolution (AdaBins / Depthformer v8)
  per image: metrics over crop & min_depth_eval < gt < max_depth_eval,
             pred clamped into [min_depth_eval, max_depth_eval]
  eval.align "median" / "lstsq" / "lstsq_disp" (this framework's own key,
  DESIGN.md 1c): pred is first aligned per image to its ground truth
  eval.tile (this framework's own key): pred comes from a
  TiledPredictor -- the model run on overlapping tiles, the tiles blended
  eval.boundary (this framework's own key): each image's
  scale-invariant boundary F1, precision and recall of the evaluated value
  (mdemi_depth_boundary) are reported next to the nine metrics

Every step is a libmdemi launch (flip: mdemi_flip_w / mdemi_flip_avg_w;
resize: mdemi_bilinear_*; metrics: mdemi_depth_metrics, or mdemi_depth_align +
mdemi_depth_metrics_aligned); only the per-image metric rows (B x 10 fp64,
B x 12 with the alignment's s and t) come back to the host.
"""

import torch

from . import functional as mf
from .utils.common_utils import RunningAverageDict
from .utils.depth_utils import tcompute_errors_gpu
from .utils.dist_utils import all_reduce_dict

__all__ = ["predict_depth", "evaluate_batch", "evaluate", "MetricMeans", "GraphedPredictor", "TiledPredictor"]


def _depth_of(out):
    # NewCRFDepth -> depth; UnetAdaptiveBins -> (pred, bin_edges); DepthformerV8 -> (depth, centers, attn)
    return out[0] if isinstance(out, (tuple, list)) else out


def predict_depth(model, img, flip_eval=False, size=None):
    """Depth (B,1,H,W) for an NCHW image batch; flip-eval averages in the flipped pass; `size`
    resizes the prediction (bilinear, align_corners=True) to the ground-truth resolution."""
    with torch.no_grad():
        pred = _depth_of(model(img))
        if flip_eval:
            pred = mf.flip_avg_w(pred, _depth_of(model(mf.flip_w(img))))
        if size is not None and tuple(pred.shape[-2:]) != tuple(size):
            B, _, h, w = pred.shape
            pred = mf.interpolate_bilinear(pred.reshape(B, h, w, 1), size=tuple(size),
                                           align_corners=True).reshape(B, 1, *size)
    return pred


def evaluate_batch(model, img, gt, eval_opt, data_type):
    """Per-image metric dicts (the reference's keys) for one batch.  `model` may be a
    GraphedPredictor (its capture fixes flip_eval) or a TiledPredictor."""
    if isinstance(model, (GraphedPredictor, TiledPredictor)):
        pred = model(img)
        if tuple(pred.shape[-2:]) != tuple(gt.shape[-2:]):
            B, _, h, w = pred.shape
            pred = mf.interpolate_bilinear(pred.reshape(B, h, w, 1), size=tuple(gt.shape[-2:]),
                                           align_corners=True).reshape(B, 1, *gt.shape[-2:])
    else:
        pred = predict_depth(model, img, bool(eval_opt.get("flip_eval", False)), size=tuple(gt.shape[-2:]))
    return tcompute_errors_gpu(pred, gt, eval_opt, data_type)


class GraphedPredictor:
    """Inference (model forward, + the flipped pass and average when flip_eval) captured once into
    a hipGraph (torch.cuda.CUDAGraph) for a fixed input shape and replayed per batch: one graph
    launch instead of ~1000 kernel launches.  Every kernel is a libmdemi launch on the capturing
    stream; workspaces come from torch's allocator (the graph's private pool) and nothing on the
    path synchronises with the host.  Eval mode only: no dropout / drop-path seeds are baked in.
    Warm-up runs happen before capture so the GEMM autotuner has settled on every shape."""

    def __init__(self, model, example_img, flip_eval=False, warmup=2):
        if model.training:
            raise ValueError("GraphedPredictor needs model.eval() (training draws host-side RNG seeds)")
        self.model, self.flip_eval = model, bool(flip_eval)
        self.static_in = example_img.detach().clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                predict_depth(model, self.static_in, self.flip_eval)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        from .train.builder import quiesce_process_group
        quiesce_process_group()  # no eager collective may be polled by the watchdog mid-capture
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_out = predict_depth(model, self.static_in, self.flip_eval)

    def __call__(self, img):
        if img.shape != self.static_in.shape:
            raise ValueError(f"GraphedPredictor captured {tuple(self.static_in.shape)}, got {tuple(img.shape)}")
        self.static_in.copy_(img)
        self.graph.replay()
        return self.static_out.clone()


class TiledPredictor:
    """Sliding-window inference (cfg eval.tile): callable like predict_depth,
    (B,3,H,W) -> (B,1,H,W) at the image's size, whatever that is.  The image is cut into tiles of
    `tile` overlapping by `overlap` (functional.tile_plan / tile_extract, one launch), the tiles go
    through the model `tile_batch` at a time (all at once when None), and functional.tile_merge
    blends the per-tile predictions with a ramp over the overlaps -- with align "lstsq" /
    "lstsq_disp" after fitting each tile's scale and shift to the tiles before it, for models whose
    depth is only defined up to those (max_depth bounds the "lstsq_disp" result).  An axis on
    which the image is no larger than the tile has one tile, clipped to the image.

    `model` is an nn.Module in eval mode or a GraphedPredictor captured at (tile_batch, 3, th, tw):
    its capture fixes flip_eval and tile_batch, a last chunk that is short is filled by repeating
    its final tile and the filling dropped, so images of every size replay the one graph.
    Half-resolution heads are resized per tile to the tile (bilinear, align_corners=True) before
    the merge.  `coef` keeps the last call's (B,T,4) fit rows (None under align "none")."""

    def __init__(self, model, tile, overlap, align="none", max_depth=None, flip_eval=False, tile_batch=None):
        from .utils.depth_utils import _pair, check_tile_align
        self.model, self.align, self.max_depth = model, check_tile_align(align, "align"), max_depth
        self.tile, self.overlap = _pair(tile, "tile", 1), _pair(overlap, "overlap", 0)
        if self.align == "lstsq_disp" and not (max_depth is not None and max_depth > 0):
            raise ValueError(f"align 'lstsq_disp' needs max_depth > 0, got {max_depth!r}")
        self.graphed = isinstance(model, GraphedPredictor)
        if self.graphed:
            captured = tuple(model.static_in.shape)
            if tile_batch is None:
                tile_batch = captured[0]
            if captured != (tile_batch, 3, *self.tile):
                raise ValueError(f"TiledPredictor: the GraphedPredictor captured {captured}, the tiles come as "
                                 f"{(tile_batch, 3, *self.tile)}")
            flip_eval = model.flip_eval
        if tile_batch is not None and (isinstance(tile_batch, bool) or not isinstance(tile_batch, int) or tile_batch < 1):
            raise ValueError(f"tile_batch must be a positive integer, got {tile_batch!r}")
        self.flip_eval, self.tile_batch = bool(flip_eval), tile_batch
        self.coef, self._plans = None, {}

    # evaluate() switches its model to eval mode and back
    @property
    def training(self):
        return False if self.graphed else self.model.training

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        if not self.graphed:
            self.model.train(mode)
        return self

    def plan(self, H, W):
        """The tile plan of an H x W image; the overlap is dropped on an axis that has one tile."""
        p = self._plans.get((H, W))
        if p is None:
            overlap = tuple(0 if n <= t else o for n, t, o in zip((H, W), self.tile, self.overlap))
            p = self._plans[(H, W)] = mf.tile_plan(H, W, self.tile, overlap)
        return p

    def __call__(self, img):
        if img.dim() != 4:
            raise ValueError(f"TiledPredictor: img must be (B,3,H,W), got {tuple(img.shape)}")
        H, W = img.shape[-2:]
        plan = self.plan(H, W)
        with torch.no_grad():
            tiles = mf.tile_extract(img.detach(), plan)
            n_all = tiles.shape[0]
            step = self.tile_batch or n_all
            preds = []
            for i in range(0, n_all, step):
                chunk = tiles[i:i + step]
                n = chunk.shape[0]
                if self.graphed:
                    if n < step:  # the captured shape: repeat the final tile, drop its predictions below
                        chunk = torch.cat([chunk, chunk[-1:].expand(step - n, -1, -1, -1)])
                    pred = self.model(chunk)
                    if tuple(pred.shape[-2:]) != plan.tile:
                        h, w = pred.shape[-2:]
                        pred = mf.interpolate_bilinear(pred.reshape(step, h, w, 1), size=plan.tile,
                                                       align_corners=True).reshape(step, 1, *plan.tile)
                else:
                    pred = predict_depth(self.model, chunk, self.flip_eval, size=plan.tile)
                preds.append(pred[:n])
            pred = preds[0] if len(preds) == 1 else torch.cat(preds)
            depth, self.coef = mf.tile_merge(pred, plan, (H, W), self.align, self.max_depth)
        return depth


class MetricMeans:
    """The means evaluate() returns, from per-image metric dicts: the nine metrics exactly as the
    reference's RunningAverageDict and all_reduce_dict make them, and -- with boundary=True (cfg
    eval.boundary) -- the boundary scores beside them with a sum and a count of their own, since an
    image without a boundary score (no BOUNDARY_KEYS in its dict) counts in the nine and not there."""

    def __init__(self, boundary=False):
        from .utils.depth_utils import BOUNDARY_KEYS
        self.boundary, self.keys = bool(boundary), BOUNDARY_KEYS
        self.avg, self.n = RunningAverageDict(), 0
        self.edge_sum, self.edge_n = {k: 0.0 for k in BOUNDARY_KEYS}, 0

    def update(self, m):
        if all(k in m for k in self.keys):
            for k in self.keys:
                self.edge_sum[k] += float(m[k])
            self.edge_n += 1
        self.avg.update({k: v for k, v in m.items() if k not in self.keys})
        self.n += 1

    def result(self, weight_by_count=False):
        """The nine means (the unweighted rank mean, or the (sum, count) reduction under
        weight_by_count), then under boundary the three boundary means -- always reduced across
        ranks as (sum, count); absent when no image on any rank had a score -- and boundary_images,
        the number of images that had one.  Every rank makes the same collective calls."""
        if not weight_by_count:
            out = all_reduce_dict(self.avg.get_value(), op="mean")
        else:
            from .utils.depth_utils import METRICS
            n = self.n
            vals = self.avg.get_value() if n else {k: 0.0 for k in METRICS}  # every rank reduces the same keys
            sums = {k: float(v) * n for k, v in vals.items()}
            tot = all_reduce_dict({"__count": float(n), **sums}, op="sum")
            count = tot.pop("__count")
            out = {k: v / count for k, v in tot.items()}
        if self.boundary:
            tot = all_reduce_dict({"__count": float(self.edge_n), **self.edge_sum}, op="sum")
            count = int(round(float(tot.pop("__count"))))
            if count:
                out.update({k: float(v) / count for k, v in tot.items()})
            out["boundary_images"] = count
        return out


def evaluate(model, batches, eval_opt, data_type, weight_by_count=False):
    """Running mean of the metrics over (img, gt) batches on this rank, then the mean over ranks
    (all_reduce_dict op="mean"; a pass-through without a process group).

    The rank mean is unweighted, as all_reduce_dict(op="mean") makes it: exact when every
    rank sees the same number of images (a padded DistributedSampler).  weight_by_count=True
    instead reduces (sum, count) per metric and divides once -- the exact dataset mean when
    ranks see different numbers of images (uneven last batch, no padding).

    With eval.boundary the result also carries the boundary scores, each the mean over the images
    that have one (MetricMeans), and boundary_images, their number."""
    from .utils.depth_utils import check_boundary
    was_training = model.training
    model.eval()
    means = MetricMeans(boundary=check_boundary(eval_opt.get("boundary")) is not None)
    try:
        for img, gt in batches:
            for m in evaluate_batch(model, img, gt, eval_opt, data_type):
                means.update(m)
    finally:
        model.train(was_training)
    return means.result(weight_by_count)
