"""Time the scale- and shift-invariant loss (mdemi_ssi_fwd / _bwd) against SILog on the same tensors.

    python tools/ssi_bench.py [--sets 12] [--rounds 4] [--spaces depth disp] [--trims 0 0.2]

The yardstick is the SILog forward + backward pair (20 B/pixel: the forward reads pred and gt, the
backward reads both and writes dpred).  The SSI pair moves 28 B/pixel without trimming (two forward
sweeps and the backward) and 48 B/pixel with it (the select's first pass also writes the 4-byte rho
plane, its other two passes read only that plane).  Cases: NYU 8x480x640, KITTI 8x352x704, and KITTI
with 5 % of the ground truth valid.  The calls go through the C ABI and are captured in hipGraphs (no
host time between launches); each graph walks --sets independent (pred, gt, dpred) triples, so that
no launch finds its inputs in the 256 MiB Infinity Cache, --rounds times.  Windows of 20 replays are
event-timed, alternating between the graphs of one case; the median of 7 windows is reported with
its min and max.  The per-launch cost of the same session comes from a graph of SILog forwards on a
64-pixel tensor (two launches each, no work).  Prints one JSON line per (case, space, trim):
microseconds per call, the ratio to SILog's pair, the byte ratio, the launch counts, and what is
left of the ratio's excess over the byte ratio after launches x the per-launch cost.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monocular-depth-estimation_amd"))

CASES = [("nyu", 8, 480, 640, 1.0), ("kitti", 8, 352, 704, 1.0), ("kitti_sparse", 8, 352, 704, 0.05)]
SILOG_BYTES, SILOG_LAUNCHES = 20, 3  # partial, finalize; backward


def ssi_bytes(trimmed):
    return 48 if trimmed else 28


def ssi_launches(trimmed):
    # moments, solve, resid, finalize, backward; trimmed: + clear, 3 x (histogram, select)
    return 12 if trimmed else 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--spaces", nargs="+", default=["depth", "disp"], choices=["depth", "disp"])
    ap.add_argument("--trims", type=float, nargs="+", default=[0.0, 0.2])
    ap.add_argument("--cases", nargs="+", default=[c[0] for c in CASES], choices=[c[0] for c in CASES])
    ap.add_argument("--windows", type=int, default=7, help="timed windows per graph (the median is reported)")
    ap.add_argument("--replays", type=int, default=20, help="graph replays per window; a kernel-trace run "
                                                            "wants few of both")
    args = ap.parse_args()
    from mdemi import _lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    md = 1e-3
    loss = torch.empty(1, device=dev)
    dloss = torch.ones(1, device=dev)

    def graph_of(sets, rounds, *fns):
        for s in sets:  # eager warm-up: code objects loaded, stats / coef written
            for f in fns:
                f(*s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(rounds):
                for s in sets:
                    for f in fns:
                        f(*s)
        return gr

    def measure(graphs, calls):
        for gr in graphs.values():
            for _ in range(3):
                gr.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in graphs}
        for _ in range(args.windows):  # windows alternate between the graphs
            for k, gr in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.replays):
                    gr.replay()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3 / (args.replays * calls[k]))
        return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}

    for name, B, H, W, keep in CASES:
        if name not in args.cases:
            continue
        HW = H * W
        g = torch.Generator(device=dev).manual_seed(0)
        sets = []
        for _ in range(args.sets):
            gt = torch.rand(B, 1, H, W, device=dev, generator=g) * 9.0 + 0.5
            gt[torch.rand(B, 1, H, W, device=dev, generator=g) >= keep] = 0.0
            pred = gt.clamp_min(0.5) * torch.exp(torch.rand(B, 1, H, W, device=dev, generator=g) - 0.5)
            sets.append((pred, gt, torch.empty_like(pred)))
        stats = torch.empty(B, 4, device=dev)
        coef = torch.empty(B, 8, device=dev, dtype=torch.float64)
        ws_s = torch.empty(max(lib.mdemi_silog_workspace_size(B, HW), 256), dtype=torch.uint8, device=dev)
        ws_i = torch.empty(max(lib.mdemi_ssi_workspace_size(B, H, W, 1), 256), dtype=torch.uint8, device=dev)
        tiny = torch.ones(64, device=dev)

        def silog_fwd(p, t, d):
            L.check(lib.mdemi_silog_fwd(p.data_ptr(), t.data_ptr(), loss.data_ptr(), stats.data_ptr(), B, HW, md,
                                        10.0, 0.15, 0, 0, ws_s.data_ptr(), L.stream()), "silog_fwd")

        def silog_bwd(p, t, d):
            L.check(lib.mdemi_silog_bwd(p.data_ptr(), t.data_ptr(), stats.data_ptr(), dloss.data_ptr(), d.data_ptr(),
                                        B, HW, md, 10.0, 0.15, 0, 0, L.stream()), "silog_bwd")

        def launch_pair(p, t, d):  # two launches over 64 pixels: the cost of launching, nothing else
            L.check(lib.mdemi_silog_fwd(tiny.data_ptr(), tiny.data_ptr(), loss.data_ptr(), stats.data_ptr(), 1, 64,
                                        md, 10.0, 0.15, 0, 0, ws_s.data_ptr(), L.stream()), "silog_fwd")

        for space in args.spaces:
            code = ("depth", "disp").index(space)
            for trim in args.trims:

                def ssi_fwd(p, t, d):
                    L.check(lib.mdemi_ssi_fwd(p.data_ptr(), t.data_ptr(), loss.data_ptr(), coef.data_ptr(), B, H, W,
                                              md, code, trim, 0, 0, ws_i.data_ptr(), L.stream()), "ssi_fwd")

                def ssi_bwd(p, t, d):
                    L.check(lib.mdemi_ssi_bwd(p.data_ptr(), t.data_ptr(), coef.data_ptr(), dloss.data_ptr(),
                                              d.data_ptr(), B, H, W, md, code, L.stream()), "ssi_bwd")

                graphs = {"silog_pair": graph_of(sets, args.rounds, silog_fwd, silog_bwd),
                          "ssi_fwd": graph_of(sets, args.rounds, ssi_fwd),
                          "ssi_bwd": graph_of(sets, args.rounds, ssi_bwd),
                          "ssi_pair": graph_of(sets, args.rounds, ssi_fwd, ssi_bwd),
                          "launch": graph_of(sets, args.rounds, launch_pair)}
                calls = {k: args.rounds * args.sets for k in graphs}
                calls["launch"] *= 2  # per launch
                t = measure(graphs, calls)
                trimmed = trim > 0
                res = {"case": name, "batch": B, "hw": [H, W], "keep": keep, "space": space, "trim": trim,
                       "sets": args.sets}
                for k, (med, lo, hi) in t.items():
                    res[k + "_us"] = round(med, 3)
                    res[k + "_us_min_max"] = [round(lo, 3), round(hi, 3)]
                ratio = t["ssi_pair"][0] / t["silog_pair"][0]
                byte_ratio = ssi_bytes(trimmed) / SILOG_BYTES
                extra_launches = ssi_launches(trimmed) - SILOG_LAUNCHES
                res["ssi_over_silog"] = round(ratio, 3)
                res["byte_ratio"] = round(byte_ratio, 3)
                res["launches"] = {"silog_pair": SILOG_LAUNCHES, "ssi_pair": ssi_launches(trimmed)}
                res["silog_pair_tbps"] = round(B * HW * SILOG_BYTES / t["silog_pair"][0] * 1e-6, 3)
                res["ssi_pair_tbps"] = round(B * HW * ssi_bytes(trimmed) / t["ssi_pair"][0] * 1e-6, 3)
                # ssi_pair - (byte_ratio x silog_pair + the extra launches at this session's cost)
                res["unexplained_us"] = round(t["ssi_pair"][0] - byte_ratio * t["silog_pair"][0]
                                              - extra_launches * t["launch"][0], 3)
                print(json.dumps(res), flush=True)
                del graphs
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
