"""Time the aligned depth metrics (mdemi_depth_align + mdemi_depth_metrics_aligned, cfg eval.align)
against the unaligned mdemi_depth_metrics on the same tensors.

    python tools/align_bench.py [--batch 8] [--hw 480 640] [--keep 1.0] [--sets 16] [--rounds 2]

The unaligned call reads gt everywhere and pred where gt is valid: one sweep, the yardstick.  By
bytes a least-squares mode is two such sweeps (sums, then metrics) and the median four (one per
select pass, then metrics).  The calls go through the C ABI and are captured in hipGraphs (no host
time between launches); each graph walks --sets independent (pred, gt) pairs so that no launch
finds its inputs in the 256 MiB Infinity Cache (16 x 19.7 MB at NYU 8x480x640), --rounds times.
Windows of 20 replays are event-timed, the variants alternating; the median of 7 windows is
reported with its min and max.  Prints one JSON line: microseconds per call for the yardstick,
for each mode's pair and for its align call alone, and each pair's ratio to the yardstick.
Use --hw 352 1216 --keep 0.05 for KITTI's sparse ground truth.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monocular-depth-estimation_amd"))

MODES = ("median", "lstsq", "lstsq_disp")
SWEEPS = {"median": 4, "lstsq": 2, "lstsq_disp": 2}  # by bytes, in units of the yardstick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--keep", type=float, default=1.0, help="share of valid ground-truth pixels")
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-depth", type=float, default=80.0)
    args = ap.parse_args()
    from mdemi import _lib as L
    from mdemi.functional import ALIGN_CODES
    lib = L.load()
    dev = torch.device("cuda", 0)
    B, (H, W) = args.batch, args.hw
    rect = (int(0.05 * H), int(0.95 * H), int(0.04 * W), int(0.96 * W))
    dmin, dmax = 1e-3, args.max_depth
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(args.sets):
        gt = torch.exp(torch.rand(B, 1, H, W, device=dev, generator=g) * 4.0 - 0.7)  # 0.5 .. 27
        pred = (0.37 * gt + 1.9) * torch.exp(0.1 * torch.randn(B, 1, H, W, device=dev, generator=g))
        gt[torch.rand(B, 1, H, W, device=dev, generator=g) >= args.keep] = 0.0
        sets.append((pred, gt))
    out10 = torch.empty(B, 10, device=dev, dtype=torch.float64)
    out12 = torch.empty(B, 12, device=dev, dtype=torch.float64)
    coef = torch.empty(B, 4, device=dev, dtype=torch.float64)
    ws_m = torch.empty(max(lib.mdemi_depth_metrics_workspace_size(B, H, W), 256), dtype=torch.uint8, device=dev)
    ws_a = {m: torch.empty(max(lib.mdemi_depth_align_workspace_size(B, H, W, c), 256), dtype=torch.uint8, device=dev)
            for m, c in ALIGN_CODES.items()}

    def metrics(p, t):
        L.check(lib.mdemi_depth_metrics(p.data_ptr(), t.data_ptr(), B, H, W, *rect, dmin, dmax, 1, out10.data_ptr(),
                                        ws_m.data_ptr(), L.stream()), "depth_metrics")

    def align_of(mode):
        def f(p, t):
            L.check(lib.mdemi_depth_align(p.data_ptr(), t.data_ptr(), B, H, W, *rect, dmin, dmax, ALIGN_CODES[mode],
                                          coef.data_ptr(), ws_a[mode].data_ptr(), L.stream()), "depth_align")
        return f

    def aligned_of(mode):
        def f(p, t):
            L.check(lib.mdemi_depth_metrics_aligned(p.data_ptr(), t.data_ptr(), B, H, W, *rect, dmin, dmax, 1,
                                                    ALIGN_CODES[mode], coef.data_ptr(), None, out12.data_ptr(),
                                                    ws_m.data_ptr(), L.stream()), "depth_metrics_aligned")
        return f

    def graph_of(*fns):
        for s in sets:  # eager warm-up: code objects loaded, coef written
            for f in fns:
                f(*s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(args.rounds):
                for s in sets:
                    for f in fns:
                        f(*s)
        return gr

    graphs = {"metrics": graph_of(metrics)}
    for m in MODES:
        graphs[m + "_pair"] = graph_of(align_of(m), aligned_of(m))
        graphs[m + "_align"] = graph_of(align_of(m))
    for gr in graphs.values():
        for _ in range(3):
            gr.replay()
    torch.cuda.synchronize()
    calls = args.rounds * args.sets
    times = {k: [] for k in graphs}
    for _ in range(7):  # windows alternate between the graphs
        for k, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                gr.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / (20 * calls))
    res = {"batch": B, "hw": [H, W], "keep": args.keep, "sets": args.sets, "rounds": args.rounds}
    for k, v in times.items():
        res[k + "_us"] = round(sorted(v)[3], 3)
        res[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    for m in MODES:
        ratios = sorted(p / y for p, y in zip(times[m + "_pair"], times["metrics"]))  # window by window
        res[m + "_over_metrics"] = round(ratios[3], 3)
        res[m + "_over_metrics_min_max"] = [round(ratios[0], 3), round(ratios[-1], 3)]
        res[m + "_sweeps_by_bytes"] = SWEEPS[m]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
