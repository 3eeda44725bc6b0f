"""Tiled inference's cost: tile_extract, tile_align and tile_blend timed with
device events at the KITTI shape (352x1216 from 352x704 tiles, overlap 192) and a 1024x1536 frame
from 480x640 tiles, batch 1 and 4, beside the same merge written with torch ops (a weight-map
index_add, or slice adds, into a canvas, then a divide) and one tile's forward of NeW-CRFs-L07.
Windows of 50 calls (20 for the torch merges, 5 for the forward), the median, lowest and highest
of 7 (5) windows in microseconds.

    python tools/tile_bench.py [OUT.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "monocular-depth-estimation_amd")]

import numpy as np
import torch

import mdemi.functional as mf
from mdemi import _lib as L

DEV = torch.device("cuda", 0)


def timed(fn, iters=50, warm=10, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)  # us
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def torch_merge_setup(plan, B):
    th, tw = plan.tile
    H, W = plan.size
    from mdemi.utils.depth_utils import tile_weights
    wy, wx = tile_weights(plan)
    w = torch.from_numpy((wy[:, None] * wx[None, :]).astype(np.float32)).to(DEV)
    idx = []
    for y in plan.ys:
        for x in plan.xs:
            yy = torch.arange(y, y + th, device=DEV)[:, None] * W + torch.arange(x, x + tw, device=DEV)[None, :]
            idx.append(yy.reshape(-1))
    den = torch.zeros(H * W, device=DEV)
    for i in idx:
        den.index_add_(0, i, w.reshape(-1))
    return w, idx, den


def main():
    res = {}
    shapes = {"kitti_352x1216_tile352x704_ov192": ((352, 1216), (352, 704), (0, 192)),
              "frame_1024x1536_tile480x640_ov120x160": ((1024, 1536), (480, 640), (120, 160))}
    lib = L.load()
    for name, (size, tile, ov) in shapes.items():
        plan = mf.tile_plan(*size, tile, ov)
        T = len(plan.ys) * len(plan.xs)
        for B in (1, 4):
            r = {"T": T, "B": B}
            img = torch.randn(B, 3, *size, device=DEV)
            tiles = torch.rand(B * T, 1, *plan.tile, device=DEV) * 8 + 1
            r["extract"] = timed(lambda: mf.tile_extract(img, plan))
            r["merge_none(blend)"] = timed(lambda: mf.tile_merge(tiles, plan, size))
            r["merge_lstsq(align+blend)"] = timed(lambda: mf.tile_merge(tiles, plan, size, align="lstsq"))
            r["merge_lstsq_disp(align+blend)"] = timed(
                lambda: mf.tile_merge(tiles, plan, size, align="lstsq_disp", max_depth=80.0))
            # align alone
            coef = torch.empty(B, T, 4, device=DEV, dtype=torch.float64)
            ws = torch.empty(lib.mdemi_tile_align_workspace_size(B, *plan.tile), device=DEV, dtype=torch.uint8)
            pa = mf._plan_args(plan)
            t3 = tiles[:, 0].contiguous()

            def align_only():
                L.check(lib.mdemi_tile_align(t3.data_ptr(), B, *size, *plan.tile, *plan.overlap, *pa, L.ALIGN_LSTSQ,
                                             coef.data_ptr(), ws.data_ptr(), L.stream()), "align")
            r["align_lstsq_alone"] = timed(align_only)
            out = torch.empty(B, 1, *size, device=DEV)

            def blend_coef():
                L.check(lib.mdemi_tile_blend(t3.data_ptr(), coef.data_ptr(), B, *size, *plan.tile, *plan.overlap, *pa,
                                             L.ALIGN_LSTSQ, 80.0, out.data_ptr(), L.stream()), "blend")
            r["blend_lstsq_alone"] = timed(blend_coef)
            # torch merges (fp32)
            w, idx, den = torch_merge_setup(plan, B)

            def torch_index_add():
                num = torch.zeros(B, size[0] * size[1], device=DEV)
                for k in range(T):
                    num.index_add_(1, idx[k], (t3[k::T] * w).reshape(B, -1))
                return (num / den).reshape(B, 1, *size)

            def torch_slices():
                num = torch.zeros(B, *size, device=DEV)
                th, tw = plan.tile
                k = 0
                for y in plan.ys:
                    for x in plan.xs:
                        num[:, y:y + th, x:x + tw] += t3[k::T] * w
                        k += 1
                return (num / den.reshape(size))[:, None]
            got = mf.tile_merge(tiles, plan, size)[0]
            r["torch_maxdiff_vs_kernel"] = float((torch_index_add() - got).abs().max())
            r["torch_index_add_merge"] = timed(torch_index_add, iters=20, warm=5)
            r["torch_slice_add_merge"] = timed(torch_slices, iters=20, warm=5)
            r["bytes_extract"] = 2 * 4 * 3 * B * T * plan.tile[0] * plan.tile[1]
            r["bytes_blend"] = 4 * B * (T * plan.tile[0] * plan.tile[1] + size[0] * size[1])
            res[f"{name}_B{B}"] = r
            print(name, B, json.dumps(r), flush=True)
    # one tile's forward of the flagship model
    from mdemi.evaluate import predict_depth
    from mdemi.model.NewCRFs import NewCRFDepth
    torch.manual_seed(0)
    m = NewCRFDepth(version="large07", max_depth=80.0, drop_path_rate=0.0).to(DEV).eval()
    for tile in ((352, 704), (480, 640)):
        x = torch.randn(1, 3, *tile, device=DEV)
        res[f"forward_large07_{tile[0]}x{tile[1]}"] = timed(lambda: predict_depth(m, x), iters=5, warm=3, reps=5)
        print(tile, json.dumps(res[f"forward_large07_{tile[0]}x{tile[1]}"]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
