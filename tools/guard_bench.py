"""Cost of the guarded AdamW step (train.nonfinite: "skip") and of the step that keeps averaged
weights (train.ema_decay) over the NeW-CRFs-L parameter table.

Times, with HIP events around single calls, the update entry points of csrc/misc.hip on
synthetic tensors of the model's parameter shapes (270 M elements): the unguarded step, the
guarded step with finite gradients, the guarded step that skips, and mdemi_grad_sumsq alone
(what "skip" adds per step when the clip is off and nothing else needs the scalar), and the
steps with an average for every tensor (mdemi_adamw_step_ema16 / mdemi_adamw_step_dev_ema16,
unguarded and guarded): one more 4-B read and write per parameter, 36 B against 28 (38 against
30 with --b16, which gives every tensor a maintained bf16 copy in all variants).  The
variants alternate inside every round, after a warm-up; the median over the rounds is reported
with the 10th / 90th percentile, one JSON line per variant and one with the ratios.

    python tools/guard_bench.py [--version large07] [--rounds 100] [--warmup 10] [--b16]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monocular-depth-estimation_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--version", default="large07")
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--b16", action="store_true", help="every tensor also has a bf16 copy the update writes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guard_bench: needs a GPU")
    from mdemi import _lib as L
    from mdemi.model.NewCRFs import NewCRFDepth
    lib = L.load()
    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        shapes = [p.numel() for p in NewCRFDepth(version=args.version, max_depth=10.0).parameters()]
    g = torch.Generator(device=dev).manual_seed(0)
    p = [torch.randn(n, device=dev, generator=g) * 0.02 for n in shapes]
    gr = [torch.randn(n, device=dev, generator=g) * 1e-3 for n in shapes]
    m = [torch.zeros(n, device=dev) for n in shapes]
    v = [torch.zeros(n, device=dev) for n in shapes]
    chunk = lib.mdemi_multi_tensor_chunk()
    refs = (L.TensorRef * len(shapes))()
    items_t, items_c = [], []
    for i, n in enumerate(shapes):
        r = refs[i]
        r.param, r.grad, r.exp_avg, r.exp_avg_sq = p[i].data_ptr(), gr[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr()
        r.numel, r.group, r.step_slot = n, 0, i
        nch = max(1, math.ceil(n / chunk))
        items_t += [i] * nch
        items_c += list(range(nch))
    nt, ni = len(shapes), len(items_t)
    table = torch.frombuffer(bytearray(bytes(refs)), dtype=torch.uint8).to(dev)
    ws = torch.zeros(lib.mdemi_grad_norm_workspace_size(ni) // 4, dtype=torch.int32)
    ws[:2 * ni] = torch.tensor(items_t + items_c, dtype=torch.int32)
    ws = ws.to(dev)
    ema = [t.clone() for t in p]
    ematab = torch.tensor([t.data_ptr() for t in ema], dtype=torch.int64).to(dev)
    ema_state = torch.zeros(1, dtype=torch.int32, device=dev)
    p16 = [t.to(torch.bfloat16) for t in p] if args.b16 else None
    p16tab = torch.tensor([t.data_ptr() for t in p16], dtype=torch.int64).to(dev) if args.b16 else None
    b16 = p16tab.data_ptr() if args.b16 else None
    tsteps = torch.zeros(nt, dtype=torch.int32, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    guard = torch.tensor([0, 0, -1, 0], dtype=torch.int32).to(dev)
    sched = torch.tensor([2e-5, 0.9, 0.999, 1e-8, 0.01, 0.0], dtype=torch.float32).to(dev)
    groups = (L.AdamWGroup * 1)()
    groups[0].lr, groups[0].beta1, groups[0].beta2, groups[0].eps, groups[0].weight_decay = 2e-5, 0.9, 0.999, 1e-8, 0.01
    sq_ok = torch.zeros(1, device=dev)
    sq_scratch = torch.zeros(1, device=dev)
    sq_bad = torch.full((1,), float("inf"), device=dev)
    max_norm = 0.1
    tl, wsp, st = table.data_ptr(), ws.data_ptr(), L.stream()
    L.check(lib.mdemi_grad_sumsq(tl, nt, ni, 1.0, sq_ok.data_ptr(), wsp, st), "grad_sumsq")

    def host(guarded, sq):
        if guarded:
            return lib.mdemi_adamw_step_guarded16(tl, nt, groups, 1, sq.data_ptr(), max_norm, 1.0, tsteps.data_ptr(),
                                                  ni, b16, guard.data_ptr(), wsp, st)
        return lib.mdemi_adamw_step16(tl, nt, groups, 1, sq.data_ptr(), max_norm, 1.0, 1, tsteps.data_ptr(), ni,
                                      b16, wsp, st)

    def devf(guarded, sq):
        if guarded:
            return lib.mdemi_adamw_step_dev_guarded16(tl, nt, sched.data_ptr(), 1, 1, step_dev.data_ptr(),
                                                      tsteps.data_ptr(), sq.data_ptr(), max_norm, 1.0, ni, b16,
                                                      guard.data_ptr(), wsp, st)
        return lib.mdemi_adamw_step_dev16(tl, nt, sched.data_ptr(), 1, 1, step_dev.data_ptr(), tsteps.data_ptr(),
                                          sq.data_ptr(), max_norm, 1.0, ni, b16, wsp, st)

    def ema_tail(guarded):
        return (ematab.data_ptr(), 0.999, 0, ema_state.data_ptr(), guard.data_ptr() if guarded else None, wsp, st)

    def ema_host(guarded, sq):
        return lib.mdemi_adamw_step_ema16(tl, nt, groups, 1, sq.data_ptr(), max_norm, 1.0, 1, tsteps.data_ptr(), ni,
                                          b16, *ema_tail(guarded))

    def ema_dev(guarded, sq):
        return lib.mdemi_adamw_step_dev_ema16(tl, nt, sched.data_ptr(), 1, 1, step_dev.data_ptr(), tsteps.data_ptr(),
                                              sq.data_ptr(), max_norm, 1.0, ni, b16, *ema_tail(guarded))

    variants = {
        "unguarded_host": lambda: host(False, sq_ok),
        "guarded_host": lambda: host(True, sq_ok),
        "guarded_host_skipped": lambda: host(True, sq_bad),
        "unguarded_dev": lambda: devf(False, sq_ok),
        "guarded_dev": lambda: devf(True, sq_ok),
        "guarded_dev_skipped": lambda: devf(True, sq_bad),
        "ema_host": lambda: ema_host(False, sq_ok),
        "ema_guarded_host": lambda: ema_host(True, sq_ok),
        "ema_dev": lambda: ema_dev(False, sq_ok),
        "ema_guarded_dev": lambda: ema_dev(True, sq_ok),
        "ema_guarded_dev_skipped": lambda: ema_dev(True, sq_bad),
        "grad_sumsq": lambda: lib.mdemi_grad_sumsq(tl, nt, ni, 1.0, sq_scratch.data_ptr(), wsp, st),
    }
    times = {k: [] for k in variants}
    for rnd in range(args.warmup + args.rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            L.check(fn(), name)
            b.record()
            b.synchronize()
            if rnd >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    assert all(torch.isfinite(t).all() for t in p[:8])
    med = {}
    for name, ts in times.items():
        ts.sort()
        med[name] = statistics.median(ts)
        print(json.dumps({"variant": name, "median_us": round(med[name], 2), "p10_us": round(ts[len(ts) // 10], 2),
                          "p90_us": round(ts[len(ts) * 9 // 10], 2), "rounds": len(ts)}))
    print(json.dumps({"model": args.version, "elements": sum(shapes), "tensors": nt, "items": ni, "b16": args.b16,
                      "ema_over_plain_host": round(med["ema_host"] / med["unguarded_host"], 4),
                      "ema_over_plain_dev": round(med["ema_dev"] / med["unguarded_dev"], 4),
                      "ema_guarded_over_guarded_host": round(med["ema_guarded_host"] / med["guarded_host"], 4),
                      "ema_guarded_over_guarded_dev": round(med["ema_guarded_dev"] / med["guarded_dev"], 4),
                      "ema_traffic_ratio": round(38 / 30 if args.b16 else 36 / 28, 4),
                      "guarded_over_unguarded_host": round(med["guarded_host"] / med["unguarded_host"], 4),
                      "guarded_over_unguarded_dev": round(med["guarded_dev"] / med["unguarded_dev"], 4),
                      "skipped_over_unguarded_host": round(med["guarded_host_skipped"] / med["unguarded_host"], 4),
                      "skipped_over_unguarded_dev": round(med["guarded_dev_skipped"] / med["unguarded_dev"], 4),
                      "grad_sumsq_over_unguarded_host": round(med["grad_sumsq"] / med["unguarded_host"], 4)}))


if __name__ == "__main__":
    main()
