"""GPU checks of the prediction export: the one-launch sweep mdemi_depth_export
(colour map, 16-bit PNG payload, fused align_corners=True resize) against the
reference's own colorize outputs (tests/golden/visualize.npz) and the NumPy
statement of the formats, and mdemi.predict.export_predictions end to end."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda", 0)


def load_golden():
    with np.load(os.path.join(HERE, "golden", "visualize.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(arrays.pop("meta").tobytes().decode())
    return [(c, arrays[c["name"] + ".in"], arrays[c["name"] + ".out"]) for c in meta["cases"]]


CASES = load_golden()
IDS = [c["name"] for c, _, _ in CASES]


def _specials_map():
    """The golden noise map x 8 (KITTI range): NaN, +-inf, +-0, denormals, 80 and its neighbours."""
    return next(d for c, d, _ in CASES if c["name"] == "kitti_jet")


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case,d,want", CASES, ids=IDS)
def test_rgba_matches_reference(case, d, want):
    import mdemi.functional as mf
    from mdemi.utils.visualize_utils import colorize
    x = torch.from_numpy(d.copy()).to(DEV)
    got = colorize(x, vmin=case["vmin"], vmax=case["vmax"], cmap=case["cmap"])
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"colorize: {(got != want).any(-1).sum()} pixels differ"
    out = mf.depth_export(x, vmin=case["vmin"], vmax=case["vmax"], lut=case["cmap"], png_scale=256.0)
    assert tuple(out["rgba"].shape) == (1,) + want.shape and out["rgba"].dtype == torch.uint8
    assert np.array_equal(_np(out["rgba"])[0], want), "depth_export rgba"
    assert np.array_equal(_np(out["depth"])[0, 0], d[0], equal_nan=True)


@pytest.mark.parametrize("scale", [256.0, 1000.0])
def test_raw16_matches_numpy_formula(scale):
    import mdemi.functional as mf
    from mdemi.utils.visualize_utils import raw16_numpy
    d = _specials_map()
    assert np.isnan(d).any() and np.isinf(d).any() and (d < 0).any() and (d * np.float32(scale) > 65535).any()
    got = mf.depth_export(torch.from_numpy(d.copy()).to(DEV), png_scale=scale, outputs=("raw16",))["raw16"]
    assert got.dtype == torch.uint16 and tuple(got.shape) == d.shape
    want = np.minimum(np.float32(65535), np.rint(d * np.float32(scale)))
    want = np.where(d > 0, want, np.float32(0)).astype(np.uint16)
    assert np.array_equal(raw16_numpy(d, scale), want)
    assert np.array_equal(_np(got), want)


def _tile(shape):
    """A batch of the given (B, H, W) cut from the specials map (tiled as needed), each image shifted."""
    B, H, W = shape
    flat = np.resize(_specials_map().reshape(-1), B * H * W + B)
    return np.stack([flat[b:b + H * W].reshape(H, W) for b in range(B)]).astype(np.float32)


@pytest.mark.parametrize("shape", [(3, 37, 53), (1, 1, 1), (2, 8, 64)], ids=["3x37x53", "1x1x1", "2x8x64"])
def test_shapes_and_output_subsets(shape):
    """Odd widths (later images start off the 4-pixel grid), a single pixel, a fully aligned
    batch; every subset of the outputs gives the bytes it gives in the full call."""
    import itertools

    import mdemi.functional as mf
    from mdemi.utils.visualize_utils import colorize_numpy, colormap_lut, raw16_numpy
    d = _tile(shape)
    if shape == (1, 1, 1):
        d[...] = 3.5
    x = torch.from_numpy(d).to(DEV)
    kw = dict(vmin=0, vmax=80, lut="jet", png_scale=256.0)
    full = {k: _np(v) for k, v in mf.depth_export(x, **kw).items()}
    assert np.array_equal(full["depth"][:, 0], d, equal_nan=True)
    assert np.array_equal(full["rgba"], colorize_numpy(d, 0, 80, colormap_lut("jet")))
    assert np.array_equal(full["raw16"], raw16_numpy(d, 256.0))
    names = ("depth", "rgba", "raw16")
    for r in (1, 2):
        for sub in itertools.combinations(names, r):
            part = mf.depth_export(x, outputs=sub, **kw)
            assert tuple(part) == sub
            for k in sub:
                assert np.array_equal(_np(part[k]), full[k], equal_nan=True), (sub, k)


def test_unaligned_views_take_the_scalar_path():
    """Outputs are fresh allocations (aligned); a prediction that is a 4-byte-offset view is not."""
    import mdemi.functional as mf
    from mdemi.utils.visualize_utils import raw16_numpy
    d = _tile((2, 8, 64))
    buf = torch.zeros(d.size + 1, device=DEV)
    buf[1:] = torch.from_numpy(d.reshape(-1)).to(DEV)
    x = buf[1:].view(2, 8, 64)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    out = mf.depth_export(x, vmin=0, vmax=80, lut="jet", png_scale=1000.0)
    assert np.array_equal(_np(out["depth"])[:, 0], d, equal_nan=True)
    assert np.array_equal(_np(out["raw16"]), raw16_numpy(d, 1000.0))


@pytest.mark.parametrize("src,dst", [((9, 13), (37, 53)), ((18, 27), (36, 54))], ids=["9x13-37x53", "18x27-36x54"])
def test_fused_resize(src, dst):
    """depth_out agrees with interpolate_bilinear(align_corners=True) to 4 * 2^-23 * max|pred|:
    three nested lerps of values bounded by max|pred| (weights in [0, 1] summing to 1), with at
    most one rounding of difference each from floating-point contraction, plus one for the sum.
    rgba / raw16 are byte-identical to a no-resize export of the kernel's own depth_out."""
    import mdemi.functional as mf
    rng = np.random.default_rng(7)
    pred = torch.from_numpy(rng.uniform(-0.5, 11.0, size=(2, 1) + src).astype(np.float32)).to(DEV)
    kw = dict(vmin=1e-3, vmax=10.0, lut="magma_r", png_scale=1000.0)
    out = mf.depth_export(pred, size=dst, **kw)
    assert tuple(out["depth"].shape) == (2, 1) + dst
    want = mf.interpolate_bilinear(pred.reshape(2, *src, 1), size=dst, align_corners=True).reshape(2, 1, *dst)
    err = (out["depth"] - want).abs().max().item()
    bound = 4 * 2.0 ** -23 * pred.abs().max().item()
    print(f"fused resize {src}->{dst}: max|diff| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    again = mf.depth_export(out["depth"], **kw)
    assert torch.equal(again["depth"], out["depth"])
    assert torch.equal(again["rgba"], out["rgba"])
    assert torch.equal(again["raw16"].view(torch.int16), out["raw16"].view(torch.int16))
    white = (out["rgba"] == 255).all(-1).float().mean().item()
    assert 0.0 < white < 0.5  # the map is neither all white nor free of out-of-range pixels


def test_depth_export_argument_errors():
    import mdemi.functional as mf
    x = torch.ones(1, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        mf.depth_export(x, outputs=())
    with pytest.raises(ValueError):
        mf.depth_export(x, outputs=("rgb",))
    with pytest.raises(ValueError):
        mf.depth_export(x, outputs=("raw16",))  # no png_scale
    with pytest.raises(ValueError):
        mf.depth_export(torch.ones(1, 4, 4), outputs=("depth",))  # CPU tensor
    with pytest.raises(ValueError):
        mf.depth_export(x, lut=torch.zeros(256, 4, dtype=torch.uint8), outputs=("rgba",))  # host lut


def test_export_predictions_end_to_end(tmp_path):
    """NewCRFDepth tiny07 at 64x96, batch 2, flip-eval: 2 + 2 files whose decoded contents are
    rint(prediction * 1000) and colorize(prediction); the same files through a GraphedPredictor."""
    from PIL import Image

    from mdemi.evaluate import GraphedPredictor, predict_depth
    from mdemi.model.NewCRFs import NewCRFDepth
    from mdemi.predict import export_predictions
    from mdemi.utils.visualize_utils import colorize
    from oracle.weights import closed_form_fill, rng_array

    m = NewCRFDepth(version="tiny07", max_depth=10.0, drop_path_rate=0.0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    closed_form_fill(sd, seed=0.5, scale=0.02)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    img = torch.from_numpy(rng_array((2, 3, 64, 96), 3)).float().to(DEV)
    eval_opt = {"min_depth_eval": 1e-3, "max_depth_eval": 10.0, "flip_eval": True}
    pred = predict_depth(m, img, flip_eval=True)
    assert tuple(pred.shape) == (2, 1, 64, 96)
    want_raw = np.rint(_np(pred)[:, 0] * np.float32(1000)).astype(np.uint16)
    assert want_raw.min() > 0 and want_raw.max() < 65535

    def check(out_dir, model):
        paths = ["/scene_a/rgb_00001.jpg", "scene_b/sub/rgb_2.jpg"]
        written = export_predictions(model, [{"image": img, "image_path": paths}], str(out_dir), "NYU", eval_opt)
        rel = ["scene_a/rgb_00001.png", "scene_b/sub/rgb_2.png"]
        assert sorted(written) == sorted(str(out_dir / sub / r) for sub in ("raw", "vis") for r in rel)
        for i, r in enumerate(rel):
            raw = Image.open(out_dir / "raw" / r)
            assert raw.mode in ("I;16", "I")
            assert np.array_equal(np.asarray(raw).astype(np.uint16), want_raw[i])
            vis = np.asarray(Image.open(out_dir / "vis" / r))
            assert np.array_equal(vis, colorize(pred[i], vmin=1e-3, vmax=10.0, cmap="jet"))

    check(tmp_path / "eager", m)
    check(tmp_path / "graph", GraphedPredictor(m, img, flip_eval=True))
    # a plain (img, paths) pair, colour only
    written = export_predictions(m, [(img, ["x/a.jpg", "x/b.jpg"])], str(tmp_path / "pair"), "NYU", eval_opt,
                                 raw16=False, cmap="magma_r")
    assert sorted(written) == [str(tmp_path / "pair" / "vis" / "x" / n) for n in ("a.png", "b.png")]
    assert not (tmp_path / "pair" / "raw").exists()


def test_predict_cli(tmp_path):
    """python -m mdemi.predict (its main(), in process): config + checkpoint + a directory of
    images -> raw/ and vis/ trees; three NYU-style frames at batch 2 under --graph, so the last
    frame takes the eager path beside the captured one."""
    from PIL import Image

    from mdemi.dataset import GpuSampleTransform
    from mdemi.evaluate import predict_depth
    from mdemi.model.NewCRFs import NewCRFDepth
    from mdemi.predict import main
    from mdemi.utils.visualize_utils import colorize
    from oracle.weights import closed_form_fill

    m = NewCRFDepth(version="tiny07", inv_depth=False, max_depth=10.0, drop_path_rate=0.0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    closed_form_fill(sd, seed=0.5, scale=0.02)
    torch.save({"model": sd}, tmp_path / "w.pth")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    cfg = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
           "eval": {"min_depth_eval": 1e-3, "max_depth_eval": 10.0, "flip_eval": True}}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    rng = np.random.default_rng(11)
    data, lists = tmp_path / "data", tmp_path / "lists" / "NYU"
    (data / "kitchen").mkdir(parents=True)
    lists.mkdir(parents=True)
    frames, lines = [], []
    for i in range(3):
        rgb = rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(data / "kitchen" / f"rgb_{i}.png")
        Image.fromarray(rng.integers(500, 9000, size=(64, 96), dtype=np.uint16)).save(
            data / "kitchen" / f"sync_depth_{i}.png")
        frames.append(rgb)
        lines.append(f"/kitchen/rgb_{i}.png /kitchen/sync_depth_{i}.png 518.8579\n")
    (lists / "nyu_test.txt").write_text("".join(lines))
    out = tmp_path / "out"
    written = main(["--config", str(tmp_path / "cfg.json"), "--checkpoint", str(tmp_path / "w.pth"),
                    "--data-path", str(data), "--mode", "test", "--out", str(out), "--batch-size", "2",
                    "--list-root", str(tmp_path / "lists"), "--graph", "--loader-workers", "0"])
    assert len(written) == 6
    img = GpuSampleTransform("NYU", "test")(torch.from_numpy(np.stack(frames)),
                                            torch.zeros(3, 64, 96, dtype=torch.int16))[0]
    pred = torch.cat([predict_depth(m, img[:2], flip_eval=True), predict_depth(m, img[2:], flip_eval=True)])
    for i in range(3):
        raw = np.asarray(Image.open(out / "raw" / "kitchen" / f"rgb_{i}.png")).astype(np.uint16)
        assert np.array_equal(raw, np.rint(_np(pred[i, 0]) * np.float32(1000)).astype(np.uint16))
        vis = np.asarray(Image.open(out / "vis" / "kitchen" / f"rgb_{i}.png"))
        assert np.array_equal(vis, colorize(pred[i], vmin=1e-3, vmax=10.0, cmap="jet"))
