"""Write mdemi/data/colormaps.json: the 256 RGBA8 entries of the packaged colormaps, taken
from the locally installed matplotlib (``cmap(np.arange(256), bytes=True)``), so that
mdemi.utils.visualize_utils needs no matplotlib for them.

    python tools/make_colormaps.py [--out PATH]
"""
import argparse
import json
import os

import matplotlib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("jet", "magma", "magma_r", "viridis", "turbo")  # visualize_utils.PACKAGED_CMAPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "monocular-depth-estimation_amd", "mdemi", "data",
                                                  "colormaps.json"))
    args = ap.parse_args()
    luts = {}
    for name in NAMES:
        lut = np.ascontiguousarray(matplotlib.colormaps[name](np.arange(256), bytes=True), dtype=np.uint8)
        assert lut.shape == (256, 4), (name, lut.shape)
        luts[name] = lut
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    # text, one "rrggbbaa" entry per LUT index, so the tables diff and review like source
    doc = {"matplotlib": matplotlib.__version__,
           "maps": {name: [bytes(row).hex() for row in lut] for name, lut in luts.items()}}
    with open(args.out, "w", encoding="ascii") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"wrote {args.out}: {', '.join(NAMES)} from matplotlib {matplotlib.__version__}")


if __name__ == "__main__":
    main()
