"""Mirror of the reference's utils/visualize_utils.py: ``colorize`` (:10-29) and
``visualization`` (:32-51), byte for byte, without matplotlib on the path.

The reference normalises the map on the host and calls
``matplotlib.cm.get_cmap(cmap)(value, bytes=True)``.  Restated (all fp32, as
NumPy computes it for an fp32 map and Python-float bounds):

  x = (d - vmin) / (vmax - vmin)    vmax - vmin formed in double, rounded to fp32;
                                    x = d * 0 when vmin == vmax
  i = trunc(x * 256), 256 -> 255    Colormap.__call__: xa *= N; xa[xa == N] = N - 1
  rgba = lut[i]                     the colormap's 256 entries as bytes
  NaN -> (0, 0, 0, 0)               matplotlib's "bad" colour
  d > vmax or d < vmin -> 255       the reference's over / under masks

A CPU tensor takes this NumPy path; a device tensor takes the same arithmetic
in ``mdemi_depth_export`` (csrc/export.hip).  The five colormaps the project
uses are packaged as 256 x RGBA8 tables (``mdemi/data/colormaps.json``, written
by tools/make_colormaps.py from matplotlib); any other name needs matplotlib.

``raw16`` is this project's 16-bit PNG payload (the reference computes
saving_factor in ``visualization`` and never uses it): min(65535, rint(d *
scale)), 0 for NaN and d <= 0 -- read back by DepthDataset's ground-truth
decoding (png / saving_factor) to within 0.5 / scale.
"""
import json
import os
from os.path import join
from typing import List

import numpy as np
import torch

__all__ = ["colorize", "visualization", "colormap_lut", "colormap_lut_device", "colorize_numpy", "raw16_numpy",
           "PACKAGED_CMAPS"]

PACKAGED_CMAPS = ("jet", "magma", "magma_r", "viridis", "turbo")
_TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "data", "colormaps.json")
_luts: dict = {}
_dev_luts: dict = {}


def colormap_lut(name: str) -> np.ndarray:
    """The colormap's 256 RGBA8 entries, uint8 [256, 4] (``cmap(np.arange(256), bytes=True)``)."""
    lut = _luts.get(name)
    if lut is not None:
        return lut
    if name in PACKAGED_CMAPS:
        with open(_TABLES, "r", encoding="ascii") as f:  # 256 "rrggbbaa" entries per map
            rows = json.load(f)["maps"][name]
        lut = np.frombuffer(bytes.fromhex("".join(rows)), dtype=np.uint8).reshape(-1, 4).copy()
    else:
        try:
            import matplotlib
        except ImportError:
            raise ValueError(f"colormap {name!r} is not packaged (packaged: {', '.join(PACKAGED_CMAPS)}) "
                             "and matplotlib is not installed") from None
        try:
            cmap = matplotlib.colormaps[name]
        except KeyError:
            raise ValueError(f"unknown colormap {name!r} (packaged: {', '.join(PACKAGED_CMAPS)})") from None
        lut = np.ascontiguousarray(cmap(np.arange(256), bytes=True), dtype=np.uint8)
    if lut.shape != (256, 4):
        raise ValueError(f"colormap {name!r} has {lut.shape} entries, not (256, 4)")
    lut.setflags(write=False)
    _luts[name] = lut
    return lut


def colormap_lut_device(name: str, device) -> torch.Tensor:
    """colormap_lut(name) on ``device``, cached per (name, device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (name, device)
    t = _dev_luts.get(key)
    if t is None:
        t = torch.from_numpy(colormap_lut(name).copy()).to(device)
        _dev_luts[key] = t
    return t


def colorize_numpy(value: np.ndarray, vmin, vmax, lut: np.ndarray) -> np.ndarray:
    """colorize's arithmetic on an fp32 array of any shape -> uint8 (..., 4)."""
    d = np.asarray(value, dtype=np.float32)
    lo, hi = np.float32(vmin), np.float32(vmax)
    with np.errstate(invalid="ignore", over="ignore"):
        white = (d > hi) | (d < lo)
        if lo != hi:
            x = (d - lo) / np.float32(float(hi) - float(lo))
        else:
            x = d * np.float32(0.0)
        s = x * np.float32(256.0)
        bad = np.isnan(s)
        s = np.where(s == np.float32(256.0), np.float32(255.0), s)
        idx = np.clip(np.where(bad, np.float32(0.0), s), 0.0, 255.0).astype(np.int64)
    out = lut[idx]
    out[bad] = 0
    out[white] = 255
    return out


def raw16_numpy(value: np.ndarray, scale) -> np.ndarray:
    """The 16-bit PNG payload of an fp32 depth map: min(65535, rint(d * scale)), 0 for NaN and d <= 0."""
    d = np.asarray(value, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.minimum(np.float32(65535.0), np.rint(d * np.float32(scale)))
        r = np.where(d > 0, r, np.float32(0.0))
    return r.astype(np.uint16)


def colorize(value, vmin=10, vmax=1000, cmap='magma_r'):
    """value (1, H, W) tensor -> NumPy uint8 (H, W, 4), the reference's return down to the byte."""
    if value.is_cuda:
        from .. import functional as mf
        img = mf.depth_export(value[:1].float(), vmin=vmin, vmax=vmax, lut=cmap, outputs=("rgba",))["rgba"]
        img = img.cpu().numpy()[0]
    else:
        img = colorize_numpy(value.numpy()[0, :, :], vmin, vmax, colormap_lut(cmap))
    return img.squeeze()


def _saving_factor(data_type: str) -> int:
    data_type = data_type.lower()
    if data_type == "kitti":
        return 256
    if data_type == "nyu":
        return 1000
    raise ValueError(f"No support {data_type} dataset.")


def visualization(model_output: tuple, data_type: str, min_depth, max_depth, img_path: List[str], *,
                  out_root: str = "output/NYU/GT/train", cmap: str = "jet"):
    """Writes colorize(model_output[i][0]) to out_root/<img_path[i] with jpg -> png> (the
    reference's layout and naming; like the reference it strips a leading '/' from img_path
    in place).  out_root and cmap default to the reference's hard-coded values."""
    from PIL import Image
    _saving_factor(data_type)
    for i in range(len(img_path)):
        if img_path[i].startswith("/"):
            img_path[i] = img_path[i][1:]
        img_name = img_path[i].split("/")[-1]
        folder = join(out_root, "/".join(img_path[i].split("/")[:-1]))
        os.makedirs(folder, exist_ok=True)
        pred = model_output[i][0]
        viz = colorize(pred.unsqueeze(0), vmin=min_depth, vmax=max_depth, cmap=cmap)
        Image.fromarray(viz.squeeze()).save(folder + "/" + img_name.replace("jpg", "png"))
