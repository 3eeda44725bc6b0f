#!/usr/bin/env python
"""Throughput of the training driver (python -m mdemi.run) on bench.py's file workload:
NeW-CRFs-L07, NYU 480x640, batch 8, synthetic NYU-format frames written the way
bench.py --data synthetic-files writes them, 4 decode workers, train.print_freq 25.
Prints one JSON line: ms_per_step over the log windows after the first (the first window
holds the GEMM autotuning and workspace growth).  Compare with the unchanged
`bench.py --model newcrfs --data synthetic-files --steps K`.

  python tools/driver_bench.py [--steps 75] [--graph] [--precision bf16]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monocular-depth-estimation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def write_frames(root, n, seed, prefix, H=480, W=640):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    names = []
    for i in range(n):
        ph = rng.uniform(0, 6.28, 3)
        rgb = np.stack([127 + 80 * np.sin(xx / (37 + 11 * c) + yy / (53 - 7 * c) + ph[c]) for c in range(3)], -1)
        rgb = np.clip(rgb + rng.normal(0, 12, rgb.shape), 0, 255).astype(np.uint8)
        dep = (1000 * (0.5 + 9.0 * (xx / W) * (0.6 + 0.4 * np.sin(yy / 41 + ph[0])) ** 2)).astype(np.uint16)
        Image.fromarray(rgb).save(os.path.join(root, f"{prefix}_rgb_{i:04d}.jpg"), quality=95)
        Image.fromarray(dep).save(os.path.join(root, f"{prefix}_depth_{i:04d}.png"))
        names.append(f"/{prefix}_rgb_{i:04d}.jpg /{prefix}_depth_{i:04d}.png 518.8579\n")
    return names


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=75)
    ap.add_argument("--print-freq", type=int, default=25)
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--precision", default=None)
    args = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "ref_json", "nyu", "newcrfs", "newcrfs_github_eval.json")) as f:
        cfg = json.load(f)
    with tempfile.TemporaryDirectory(prefix="mdemi_driver_bench_") as tmp:
        data, lists = os.path.join(tmp, "data"), os.path.join(tmp, "lists", "NYU")
        os.makedirs(data)
        os.makedirs(lists)
        with open(os.path.join(lists, "nyu_train_36k.txt"), "w") as f:
            f.writelines(write_frames(data, args.files, 0, "train"))
        with open(os.path.join(lists, "nyu_test.txt"), "w") as f:
            f.writelines(write_frames(data, 2, 1, "test"))
        cfg.update(gpu_ids=[0], output_dir=os.path.join(tmp, "out"), checkpoint="")
        cfg["dataset"]["data_path"] = data
        cfg["dataloader"]["num_workers"] = args.workers
        cfg["train"].update(print_freq=args.print_freq, valid_freq=10 ** 9, epoch=10 ** 4)
        path = os.path.join(tmp, "cfg.json")
        with open(path, "w") as f:
            json.dump(cfg, f)
        from mdemi import run
        argv = ["--opt", path, "--list-root", os.path.join(tmp, "lists"), "--max-steps", str(args.steps)]
        argv += ["--graph"] if args.graph else []
        argv += ["--precision", args.precision] if args.precision else []
        code = run.main(argv)
        with open(os.path.join(tmp, "out", "log.jsonl")) as f:
            log = [json.loads(s) for s in f]
    train = [r for r in log if r["type"] == "train"]
    steady = train[1:] or train
    B = int(cfg["dataloader"]["batch_size"])
    ms = [1e3 * B / r["images_per_sec"] for r in steady]
    print(json.dumps({"driver": "mdemi.run", "exit_code": code, "steps": args.steps, "print_freq": args.print_freq,
                      "windows_ms_per_step": [round(m, 2) for m in [1e3 * B / r["images_per_sec"] for r in train]],
                      "ms_per_step": round(sum(ms) / len(ms), 2),
                      "images_per_sec": round(B * len(ms) / (sum(ms) / 1e3), 3) if ms else None,
                      "dropped": sum(r["dropped"] for r in train), "loss_last": train[-1]["loss"]}))
    return code


if __name__ == "__main__":
    sys.exit(main())
