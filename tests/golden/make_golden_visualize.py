"""Generate tests/golden/visualize.npz from the reference's utils/visualize_utils.py itself.

Run where the reference checkout and matplotlib are present (the reference is never shipped):

    python tests/golden/make_golden_visualize.py [--ref /root/reference]

The reference's ``colorize`` is imported as-is and called on the inputs below; the file
holds those inputs and its outputs.  Cases (name: map, vmin, vmax, cmap):

  noise_jet / noise_magma_r  1x37x53 fp32 uniform on [-0.5, 11), seed 0, with NaN, +inf, -inf,
                             exactly vmin, exactly vmax and their fp32 neighbours in row 0;
                             vmin 1e-3, vmax 10.0
  ramp_jet                   1x2x514: vmin + (k + {0, 1/2}) (vmax - vmin) / 256, k = 0..256, ascending in
                             row 0 and descending in row 1: every LUT index and every bin boundary;
                             same range
  kitti_jet                  the noise map x 8, integer vmin 0, vmax 80 (+-0 and the smallest denormals planted)
  degenerate_jet             the noise map with vmin == vmax == 5.0 (5.0 planted)
  defaults_magma_r           the noise map x 100 under the reference's defaults (10, 1000, magma_r),
                             10 and its neighbours planted
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def noise_map(vmin=1e-3, vmax=10.0):
    rng = np.random.default_rng(0)
    d = rng.uniform(-0.5, 11.0, size=(1, 37, 53)).astype(np.float32)
    lo, hi = np.float32(vmin), np.float32(vmax)
    inf = np.float32(np.inf)
    d[0, 0, :9] = [np.nan, inf, -inf, lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, -inf),
                   np.nextafter(hi, inf)]
    return d


def ramp_map(vmin=1e-3, vmax=10.0):
    k = np.arange(257, dtype=np.float64)
    step = (vmax - vmin) / 256.0
    up = np.stack([vmin + k * step, vmin + (k + 0.5) * step], axis=1).reshape(-1)  # 514 values, ascending
    return np.stack([up, up[::-1]]).astype(np.float32)[None]


def cases():
    noise = noise_map()
    deg = noise.copy()
    deg[0, 1, :3] = [5.0, np.nextafter(np.float32(5.0), np.float32(0)), np.nextafter(np.float32(5.0), np.float32(9))]
    inf = np.float32(np.inf)
    kitti = noise * np.float32(8.0)  # row 0 carries 80 and its neighbours; plant vmin = 0 and its own
    kitti[0, 1, :4] = [0.0, -0.0, np.nextafter(np.float32(0), inf), np.nextafter(np.float32(0), -inf)]
    dflt = noise * np.float32(100.0)  # row 0 carries 1000 and its neighbours; plant vmin = 10 and its own
    dflt[0, 1, :3] = [10.0, np.nextafter(np.float32(10), inf), np.nextafter(np.float32(10), -inf)]
    return [
        ("noise_jet", noise, 1e-3, 10.0, "jet"),
        ("noise_magma_r", noise, 1e-3, 10.0, "magma_r"),
        ("ramp_jet", ramp_map(), 1e-3, 10.0, "jet"),
        ("kitti_jet", kitti, 0, 80, "jet"),
        ("degenerate_jet", deg, 5.0, 5.0, "jet"),
        ("defaults_magma_r", dflt, 10, 1000, "magma_r"),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "visualize.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    from utils import visualize_utils as ref  # the reference module, unmodified

    import matplotlib
    arrays, meta = {}, []
    for name, d, vmin, vmax, cmap in cases():
        out = ref.colorize(torch.from_numpy(d.copy()), vmin=vmin, vmax=vmax, cmap=cmap)
        assert out.dtype == np.uint8 and out.shape == d.shape[1:] + (4,), (name, out.dtype, out.shape)
        arrays[name + ".in"] = d
        arrays[name + ".out"] = out
        white = float((out == 255).all(-1).mean())
        meta.append({"name": name, "vmin": vmin, "vmax": vmax, "cmap": cmap})
        print(f"{name}: {d.shape} vmin={vmin} vmax={vmax} {cmap}  white {100 * white:.1f} %")
    # the reference's defaults really are (10, 1000, magma_r)
    assert np.array_equal(ref.colorize(torch.from_numpy(arrays["defaults_magma_r.in"])), arrays["defaults_magma_r.out"])
    arrays["meta"] = np.frombuffer(json.dumps({"cases": meta, "matplotlib": matplotlib.__version__,
                                               "numpy": np.__version__}).encode(), dtype=np.uint8)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
