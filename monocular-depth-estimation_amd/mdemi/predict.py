"""Prediction export: image files -> depth PNGs and colour maps.

  python -m mdemi.predict --config <json> --checkpoint <file> --data-path <dir> \
         --mode test|benchmark --out <dir> [--graph] [--cmap jet] [--no-colour] [--no-raw16] \
         [--tile H W [--tile-overlap N | OY OX] [--tile-align none|lstsq|lstsq_disp]]

Per batch: the model's prediction (``evaluate.predict_depth`` or a
``GraphedPredictor``), then ONE ``mdemi_depth_export`` launch that resizes the
prediction to the input image (the half-resolution AdaBins / Depthformer
heads), colour-maps it as the reference's ``utils/visualize_utils.colorize``
does and quantises it for a 16-bit PNG.  Only the finished bytes (4 + 2 per
pixel) cross to the host, into one of two pinned buffer sets, so that batch i
is PNG-encoded by a thread pool while batch i+1 runs on the GPU.

Files: ``out_dir/raw/<image_path, .png>`` is 16-bit greyscale, depth x 256
(KITTI / ONLINE) or x 1000 (NYU), 0 = no value -- the datasets' own ground
truth convention, so ``DepthDataset`` decodes a written file back to within
0.5 / scale.  ``out_dir/vis/<same>`` is the RGBA colour map between
eval.min_depth_eval and eval.max_depth_eval.
"""
from __future__ import annotations

import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterable, List

import numpy as np
import torch

from . import functional as mf
from .evaluate import GraphedPredictor, TiledPredictor, predict_depth

__all__ = ["export_predictions", "png_scale_of", "main"]

PNG_SCALE = {"KITTI": 256.0, "ONLINE": 256.0, "NYU": 1000.0}
MAX_WORKERS = 16


def png_scale_of(data_type: str) -> float:
    try:
        return PNG_SCALE[data_type.upper()]
    except KeyError:
        raise ValueError(f"No support {data_type} dataset.") from None


def _rel_png(path: str) -> str:
    path = path.strip()
    while path.startswith("/"):
        path = path[1:]
    return os.path.splitext(path)[0] + ".png"


def _save_png(arr: np.ndarray, path: str) -> str:
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(arr).save(path)  # uint16 (H,W) -> 16-bit greyscale; uint8 (H,W,4) -> RGBA
    return path


class _HostSet:
    """One set of pinned host buffers with the event of the copy into them and the encode
    jobs reading them."""

    def __init__(self):
        self.buf, self.event, self.jobs, self.paths = {}, None, [], None

    def drain(self) -> List[str]:
        done = [j.result() for j in self.jobs]
        self.jobs = []
        return done

    def fill(self, out: dict, paths: List[str]) -> None:
        for k, t in out.items():
            b = self.buf.get(k)
            if b is None or b.shape != t.shape:
                b = self.buf[k] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            b.copy_(t, non_blocking=True)
        for k in [k for k in self.buf if k not in out]:
            del self.buf[k]
        self.event = torch.cuda.Event()
        self.event.record()
        self.paths = paths

    def encode(self, pool, out_dir: str) -> None:
        self.event.synchronize()  # the copy of this set only; the next batch keeps running
        for k, sub in (("raw16", "raw"), ("rgba", "vis")):
            if k in self.buf:
                arr = self.buf[k].numpy()
                for i, p in enumerate(self.paths):
                    self.jobs.append(pool.submit(_save_png, arr[i], os.path.join(out_dir, sub, _rel_png(p))))
        self.paths = None


def _split(batch, data_type, dev, transforms):
    """(image NCHW fp32 on the device, image paths) of a loader batch or an (img, paths) pair."""
    if isinstance(batch, dict):
        img, paths = batch["image"], batch["image_path"]
    else:
        img, paths = batch
    if img.dtype == torch.uint8:  # collate_raw's decoded (B,H,W,3) frames: the test transform
        from .dataset import GpuSampleTransform
        tf = transforms.get(data_type)
        if tf is None:
            tf = transforms[data_type] = GpuSampleTransform(data_type, "test")
        depth = batch.get("depth") if isinstance(batch, dict) else None
        if depth is None:
            depth = torch.zeros(img.shape[:3], dtype=torch.int16)
        img = tf(img, depth)[0]
    else:
        img = img.to(dev, non_blocking=True)
    paths = [paths] if isinstance(paths, str) else list(paths)
    if len(paths) != img.shape[0]:
        raise ValueError(f"{img.shape[0]} images but {len(paths)} image paths")
    return img, paths


def export_predictions(model, batches: Iterable, out_dir: str, data_type: str, eval_opt: dict, colour: bool = True,
                       raw16: bool = True, cmap: str = "jet", workers: int = 4) -> List[str]:
    """Write the model's predictions for ``batches`` under ``out_dir`` and return the written paths.

    batches: what a DataLoader over ``mdemi.dataset.DepthDataset`` (test or benchmark mode,
        ``collate_fn=collate_raw``) yields -- a dict with ``image`` and ``image_path`` -- or plain
        ``(img, paths)`` pairs; ``img`` is the normalised (B,3,H,W) fp32 batch or the decoded
        (B,H,W,3) uint8 frames (those go through the test-mode GpuSampleTransform).
    model: an nn.Module in eval mode, a GraphedPredictor (its capture fixes flip_eval) or a
        TiledPredictor (eval.tile: sliding-window inference, each file at its image's size).
    eval_opt: the config's ``eval`` block: min_depth_eval / max_depth_eval bound the colour map,
        flip_eval averages in the flipped pass.
    Predictions are written at the resolution the dataset yields (the KB-cropped 352x1216
    frame for KITTI / ONLINE); pasting them back into the uncropped frame is out of scope.
    """
    scale = png_scale_of(data_type)
    outputs = tuple(k for k, on in (("rgba", colour), ("raw16", raw16)) if on)
    if not outputs:
        raise ValueError("export_predictions: nothing to write (colour and raw16 both off)")
    vmin, vmax = float(eval_opt.get("min_depth_eval", 1e-3)), float(eval_opt.get("max_depth_eval", 10.0))
    flip = bool(eval_opt.get("flip_eval", False))
    dev = torch.device("cuda", torch.cuda.current_device())
    graphed = isinstance(model, (GraphedPredictor, TiledPredictor))  # called with the image alone
    was_training = (not isinstance(model, GraphedPredictor)) and model.training
    if was_training:
        model.eval()
    sets, written, transforms = (_HostSet(), _HostSet()), [], {}
    pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))
    try:
        prev = None
        for i, batch in enumerate(batches):
            cur = sets[i % 2]
            written += cur.drain()  # the encode jobs of batch i-2 still read these buffers
            img, paths = _split(batch, data_type.upper(), dev, transforms)
            pred = model(img) if graphed else predict_depth(model, img, flip)
            out = mf.depth_export(pred, size=tuple(img.shape[-2:]), vmin=vmin, vmax=vmax, lut=cmap, png_scale=scale,
                                  outputs=outputs)
            cur.fill(out, paths)
            if prev is not None:
                prev.encode(pool, out_dir)  # batch i-1, while batch i runs
            prev = cur
        if prev is not None:
            prev.encode(pool, out_dir)
        for s in sets:
            written += s.drain()
    finally:
        pool.shutdown(wait=True)
        if was_training:
            model.train(True)
    return written


def require_ema(state, filename: str, who: str) -> None:
    """Exit with a message unless the checkpoint dict holds averaged weights."""
    if not isinstance(state, dict) or state.get("ema_state_dict") is None:
        raise SystemExit(f"{who}: {filename!r} holds no ema_state_dict -- it was not written by a run with "
                         "train.ema_decay set; drop --ema to use its model_state_dict")


def _load_weights(model, filename: str, ema: bool = False) -> None:
    """ema: the file's averaged weights (ema_state_dict) instead of model_state_dict."""
    from .utils import checkpoint as ck
    state = ck.read_checkpoint(filename)
    if ema:
        require_ema(state, filename, "--ema")
        state = state["ema_state_dict"]
    elif isinstance(state, dict) and "model_state_dict" in state:  # utils.common_utils.save_checkpoint's file
        state = state["model_state_dict"]
    ck.load_checkpoint(model, state, strict=False)


def main(argv=None) -> List[str]:
    ap = argparse.ArgumentParser(prog="python -m mdemi.predict", description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="the run's JSON config (model.*, eval.*, dataset.data_type)")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data-path", required=True)
    ap.add_argument("--mode", choices=("test", "benchmark"), default="test")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch-size", type=int, default=None, help="default: the config's eval batch size, else 1")
    ap.add_argument("--list-root", default=None, help="directory of the train_test_inputs file lists")
    ap.add_argument("--graph", action="store_true", help="replay the prediction as a captured hipGraph")
    ap.add_argument("--ema", action="store_true", help="predict with the checkpoint's averaged weights "
                                                       "(ema_state_dict, written under train.ema_decay)")
    ap.add_argument("--tile", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="override the config's eval.tile: predict on overlapping H x W tiles of each image, blended "
                         "back to its size; with --graph one capture at the tile serves images of every size")
    ap.add_argument("--tile-overlap", type=int, nargs="+", default=None, metavar="N",
                    help="override eval.tile_overlap: one overlap for both axes, or OY OX (default: a quarter of "
                         "the tile)")
    ap.add_argument("--tile-align", default=None, choices=["none", "lstsq", "lstsq_disp"],
                    help="override eval.tile_align: fit each tile's scale and shift to the tiles before it")
    ap.add_argument("--cmap", default="jet")
    ap.add_argument("--no-colour", action="store_true")
    ap.add_argument("--no-raw16", action="store_true")
    ap.add_argument("--workers", type=int, default=4, help="PNG encoder threads (at most 16)")
    ap.add_argument("--loader-workers", type=int, default=4, help="image decoder processes (0: decode in this one)")
    args = ap.parse_args(argv)

    from .dataset import DepthDataset, collate_raw
    from .train.builder import build_model
    with open(args.config, "r", encoding="utf-8") as f:
        opt = json.load(f)
    from .run import tile_overrides
    from .train.builder import eval_tile
    tile_overrides(opt, args)
    tile = eval_tile(opt)  # a bad eval.tile / tile_overlap / tile_align / tile_batch fails here, before any GPU work
    eval_opt = dict(opt.get("eval", {}))
    data_type = opt["dataset"]["data_type"].upper()
    if not torch.cuda.is_available():
        raise RuntimeError("mdemi.predict needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    model = build_model(opt, drop_path=0.0)
    _load_weights(model, args.checkpoint, ema=args.ema)
    model.to(dev).eval()

    kw = {} if args.list_root is None else {"list_root": args.list_root}
    ds = DepthDataset(args.data_path, data_type, args.mode, img_size=opt["dataset"].get("img_size"), **kw)
    bs = args.batch_size or int(eval_opt.get("batch_size", 1))
    nw = max(0, min(int(args.loader_workers), MAX_WORKERS - 1))
    loader = torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=False, collate_fn=collate_raw, num_workers=nw,
                                         pin_memory=True, multiprocessing_context="fork" if nw else None)

    transforms = {}
    it = (_split(b, data_type, dev, transforms) for b in loader)
    rest = (args.out, data_type, eval_opt, not args.no_colour, not args.no_raw16, args.cmap, args.workers)
    flip = bool(eval_opt.get("flip_eval", False))
    if tile is not None:
        inner = model
        if args.graph:  # one capture at the tile: images of every size replay it
            tile["tile_batch"] = tile["tile_batch"] or bs
            inner = GraphedPredictor(model, torch.zeros(tile["tile_batch"], 3, *tile["tile"], device=dev), flip)
        written = export_predictions(TiledPredictor(inner, flip_eval=flip, **tile), it, *rest)
    elif not args.graph:
        written = export_predictions(model, it, *rest)
    else:
        written, first = [], next(it, None)
        if first is not None:
            predictor = GraphedPredictor(model, first[0], bool(eval_opt.get("flip_eval", False)))
            odd = []  # a last, smaller batch does not fit the captured shape: it runs eagerly

            def captured_shape():
                yield first
                for img, paths in it:
                    if img.shape == first[0].shape:
                        yield img, paths
                    else:
                        odd.append((img, paths))

            written = export_predictions(predictor, captured_shape(), *rest)
            if odd:
                written += export_predictions(model, odd, *rest)
    print(f"wrote {len(written)} files under {args.out}")
    return written


if __name__ == "__main__":
    main()
