"""Time the gradient-matching loss (mdemi_gradmatch_fwd / _bwd) against SILog on the same tensors.

    python tools/grad_match_bench.py [--batch 8] [--hw 480 640] [--sets 12] [--rounds 4]

Both losses move the same algorithmic bytes (forward reads pred and gt, 8 B/pixel; backward
reads both and writes dpred, 12 B/pixel), so SILog is the yardstick.  The calls go through the
C ABI and are captured in hipGraphs (no host time between launches); each graph walks --sets
independent (pred, gt, dpred) triples so that no launch finds its inputs in the 256 MiB Infinity
Cache (12 x 29.5 MB at NYU 8x480x640), --rounds times.  Windows of 20 replays are event-timed,
alternating between the two losses; the median of 7 windows is reported.  Prints one JSON line:
microseconds per forward, per backward and per pair for each loss, the pair's algorithmic TB/s
and its fraction of the 6.29 TB/s achievable HBM rate.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monocular-depth-estimation_amd"))

HBM_ACHIEVABLE = 6.29e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--sets", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--keep", type=float, default=1.0, help="share of valid ground-truth pixels")
    args = ap.parse_args()
    from mdemi import _lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    B, (H, W) = args.batch, args.hw
    HW = H * W
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(args.sets):
        gt = torch.rand(B, 1, H, W, device=dev, generator=g) * 9.0 + 0.5
        gt[torch.rand(B, 1, H, W, device=dev, generator=g) >= args.keep] = 0.0
        pred = gt.clamp_min(0.5) * torch.exp(torch.rand(B, 1, H, W, device=dev, generator=g) - 0.5)
        sets.append((pred, gt, torch.empty_like(pred)))
    loss = torch.empty(1, device=dev)
    dloss = torch.ones(1, device=dev)
    stats = torch.empty(B, 4, device=dev)
    wk = torch.empty(B, 4, device=dev)
    ws_s = torch.empty(max(lib.mdemi_silog_workspace_size(B, HW), 256), dtype=torch.uint8, device=dev)
    ws_g = torch.empty(max(lib.mdemi_gradmatch_workspace_size(B, H, W), 256), dtype=torch.uint8, device=dev)
    md = 1e-3

    def silog_fwd(p, t, d):
        L.check(lib.mdemi_silog_fwd(p.data_ptr(), t.data_ptr(), loss.data_ptr(), stats.data_ptr(), B, HW, md, 10.0,
                                    0.15, 0, 0, ws_s.data_ptr(), L.stream()), "silog_fwd")

    def silog_bwd(p, t, d):
        L.check(lib.mdemi_silog_bwd(p.data_ptr(), t.data_ptr(), stats.data_ptr(), dloss.data_ptr(), d.data_ptr(), B,
                                    HW, md, 10.0, 0.15, 0, 0, L.stream()), "silog_bwd")

    def gm_fwd(p, t, d):
        L.check(lib.mdemi_gradmatch_fwd(p.data_ptr(), t.data_ptr(), loss.data_ptr(), wk.data_ptr(), B, H, W, md,
                                        args.scales, 0, ws_g.data_ptr(), L.stream()), "gradmatch_fwd")

    def gm_bwd(p, t, d):
        L.check(lib.mdemi_gradmatch_bwd(p.data_ptr(), t.data_ptr(), wk.data_ptr(), dloss.data_ptr(), d.data_ptr(), B,
                                        H, W, md, args.scales, L.stream()), "gradmatch_bwd")

    def graph_of(*fns):
        for s in sets:  # eager warm-up: code objects loaded, stats / wk written
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

    graphs = {"silog_fwd": graph_of(silog_fwd), "silog_bwd": graph_of(silog_bwd),
              "silog_pair": graph_of(silog_fwd, silog_bwd),
              "gradmatch_fwd": graph_of(gm_fwd), "gradmatch_bwd": graph_of(gm_bwd),
              "gradmatch_pair": graph_of(gm_fwd, gm_bwd)}
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
    res = {"batch": B, "hw": [H, W], "scales": args.scales, "keep": args.keep, "sets": args.sets,
           "bytes_pair": B * HW * 20}
    for k, v in times.items():
        res[k + "_us"] = round(sorted(v)[3], 3)
        res[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    for name in ("silog", "gradmatch"):
        rate = res["bytes_pair"] / (res[name + "_pair_us"] * 1e-6)
        res[name + "_pair_tbps"] = round(rate / 1e12, 3)
        res[name + "_pair_hbm_fraction"] = round(rate / HBM_ACHIEVABLE, 3)
    res["gradmatch_over_silog"] = round(res["gradmatch_pair_us"] / res["silog_pair_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
