"""CPU checks of the prediction-export surface: mdemi.utils.visualize_utils against
the reference's own colorize outputs (tests/golden/visualize.npz, written by
tests/golden/make_golden_visualize.py), the packaged colormap tables, the 16-bit
PNG format, the file layout of visualization() and the C ABI's error path."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "visualize.npz")


def load_golden():
    with np.load(GOLDEN) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(arrays.pop("meta").tobytes().decode())
    return [(c, arrays[c["name"] + ".in"], arrays[c["name"] + ".out"]) for c in meta["cases"]]


CASES = load_golden()
IDS = [c["name"] for c, _, _ in CASES]


def test_golden_is_not_mostly_white():
    """Fewer than 25 % of the golden pixels of the noise, ramp and integer-range cases are
    white-outs, so painting everything white cannot pass."""
    names = {"noise_jet", "noise_magma_r", "ramp_jet", "kitti_jet"}
    outs = [o.reshape(-1, 4) for c, _, o in CASES if c["name"] in names]
    assert len(outs) == len(names)
    px = np.concatenate(outs)
    assert (px == 255).all(-1).mean() < 0.25
    assert len({c["name"] for c, _, _ in CASES}) == 6


@pytest.mark.parametrize("case,d,want", CASES, ids=IDS)
def test_colorize_cpu_matches_reference(case, d, want):
    from mdemi.utils.visualize_utils import colorize
    got = colorize(torch.from_numpy(d.copy()), vmin=case["vmin"], vmax=case["vmax"], cmap=case["cmap"])
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"{(got != want).any(-1).sum()} pixels differ"


def test_colorize_defaults_are_the_references():
    from mdemi.utils.visualize_utils import colorize
    case, d, want = next(c for c in CASES if c[0]["name"] == "defaults_magma_r")
    assert np.array_equal(colorize(torch.from_numpy(d.copy())), want)


def test_packaged_luts_match_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    from mdemi.utils.visualize_utils import PACKAGED_CMAPS, colormap_lut
    for name in PACKAGED_CMAPS:
        want = matplotlib.colormaps[name](np.arange(256), bytes=True)
        got = colormap_lut(name)
        assert got.dtype == np.uint8 and got.shape == (256, 4)
        assert np.array_equal(got, want), name


def test_packaged_luts_need_no_matplotlib(monkeypatch):
    import sys

    from mdemi.utils import visualize_utils as vu
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # import matplotlib -> ImportError
    monkeypatch.setattr(vu, "_luts", {})
    for name in vu.PACKAGED_CMAPS:
        assert vu.colormap_lut(name).shape == (256, 4)
    with pytest.raises(ValueError, match="jet"):
        vu.colormap_lut("no_such_map")


def test_raw16_semantics():
    from mdemi.utils.visualize_utils import raw16_numpy
    inf = np.float32(np.inf)
    d = np.array([np.nan, -1.0, -0.0, 0.0, -inf, inf, 1e9, 0.5, 1.5, 2.5, 3.25], dtype=np.float32)
    #                                                    256: 128, 384, 640, 832     1000: 500, 1500, 2500, 3250
    assert raw16_numpy(d, 256).tolist() == [0, 0, 0, 0, 0, 65535, 65535, 128, 384, 640, 832]
    assert raw16_numpy(d, 1000).tolist() == [0, 0, 0, 0, 0, 65535, 65535, 500, 1500, 2500, 3250]
    # round half to even on the product, saturation just past the top code
    h = np.array([0.5 / 256, 1.5 / 256, 2.5 / 256, 65534.5 / 256, 65535.5 / 256, 255.998, 256.0], dtype=np.float32)
    assert raw16_numpy(h, 256).tolist() == [0, 2, 2, 65534, 65535, 65535, 65535]
    assert raw16_numpy(np.float32([65.5342, 65.536, 80.0]), 1000).tolist() == [65534, 65535, 65535]
    assert raw16_numpy(d, 256).dtype == np.uint16


@pytest.mark.parametrize("scale", [256, 1000])
def test_raw16_png_reads_back_as_ground_truth(tmp_path, scale):
    """A written 16-bit PNG, decoded as DepthDataset decodes ground truth (uint16 / factor),
    is within 0.5 / scale of the prediction."""
    from PIL import Image

    from mdemi.utils.visualize_utils import raw16_numpy
    top = 65535.0 / scale  # the largest depth the format holds
    d = np.random.default_rng(1).uniform(1e-3, min(top, 80.0), size=(17, 23)).astype(np.float32)
    p = str(tmp_path / "d.png")
    Image.fromarray(raw16_numpy(d, scale)).save(p)
    back = np.asarray(Image.open(p)).astype(np.uint16)  # dataset.py DepthDataset.__getitem__
    assert back.shape == d.shape
    depth = back.astype(np.float64) / scale
    assert np.abs(depth - d.astype(np.float64)).max() <= 0.5 / scale


def test_visualization_writes_reference_layout(tmp_path, monkeypatch):
    from PIL import Image

    from mdemi.utils.visualize_utils import colorize, visualization
    monkeypatch.chdir(tmp_path)
    _, d, _ = next(c for c in CASES if c[0]["name"] == "noise_jet")
    preds = [torch.from_numpy(d.copy()), torch.from_numpy(d[:, ::-1].copy())]  # model_output[i][0] is (H, W)
    paths = ["/kitchen_0001/rgb_00045.jpg", "study/rgb_7.jpg"]
    visualization(tuple(preds), "NYU", 1e-3, 10.0, paths)
    assert paths == ["kitchen_0001/rgb_00045.jpg", "study/rgb_7.jpg"]  # stripped in place, as the reference does
    for pred, rel in zip(preds, ("kitchen_0001/rgb_00045.png", "study/rgb_7.png")):
        f = tmp_path / "output" / "NYU" / "GT" / "train" / rel
        assert f.is_file()
        img = np.asarray(Image.open(f))
        assert np.array_equal(img, colorize(pred, vmin=1e-3, vmax=10.0, cmap="jet"))
    visualization((preds[0],), "kitti", 1e-3, 10.0, ["a/b.jpg"], out_root=str(tmp_path / "o"), cmap="magma_r")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o" / "a" / "b.png")),
                          colorize(preds[0], vmin=1e-3, vmax=10.0, cmap="magma_r"))
    with pytest.raises(ValueError, match="No support online dataset."):
        visualization((preds[0],), "ONLINE", 1e-3, 10.0, ["a/c.jpg"])


def test_depth_export_abi_error_path():
    """An invalid call returns a negative code and a message before any launch."""
    from mdemi import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every check fails before a launch
    assert lib.mdemi_depth_export(one, 1, 4, 4, 4, 4, 0.0, 1.0, one, 256.0, None, None, None, None) < 0
    assert b"depth_export" in lib.mdemi_last_error()
    assert lib.mdemi_depth_export(None, 1, 4, 4, 4, 4, 0.0, 1.0, one, 256.0, one, None, None, None) < 0
    assert lib.mdemi_depth_export(one, 1, 0, 4, 4, 4, 0.0, 1.0, one, 256.0, one, None, None, None) < 0
    assert lib.mdemi_depth_export(one, 1, 4, 4, 4, -1, 0.0, 1.0, one, 256.0, one, None, None, None) < 0
    rc = lib.mdemi_depth_export(one, 1, 4, 4, 4, 4, 0.0, 1.0, None, 256.0, None, one, None, None)  # rgba, no lut
    assert rc < 0 and b"lut" in lib.mdemi_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc, "depth_export")


def test_export_predictions_rejects_unknown_dataset():
    from mdemi.predict import png_scale_of
    assert png_scale_of("kitti") == 256 and png_scale_of("ONLINE") == 256 and png_scale_of("nyu") == 1000
    with pytest.raises(ValueError):
        png_scale_of("cityscapes")
