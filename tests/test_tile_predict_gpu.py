"""Tiled inference end to end on the GPU: evaluate.TiledPredictor over the tiny07 NeW-CRFs (eager and
over a GraphedPredictor captured at the tile), export_predictions and python -m mdemi.predict
--tile, and python -m mdemi.run --test with eval.tile."""
import json
import math
import os

import numpy as np
import pytest
import torch

from test_run_gpu import METRICS, _config, _write_frames

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TILE, OVERLAP = (64, 96), 32


@pytest.fixture(scope="module")
def model():
    from mdemi.model.NewCRFs import NewCRFDepth
    from oracle.weights import closed_form_fill
    m = NewCRFDepth(version="tiny07", inv_depth=False, max_depth=10.0, drop_path_rate=0.0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    closed_form_fill(sd, seed=0.5, scale=0.02)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def _images(n, size=(64, 160), seed=3):
    from oracle.weights import rng_array
    return torch.from_numpy(rng_array((n, 3) + size, seed)).float().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _chunked_reference(m, img, tile_batch, pad):
    """tile_merge of predict_depth on the tiles, tile_batch at a time; pad: a short last chunk is
    filled by repeating its final tile, as a captured shape needs."""
    import mdemi.functional as mf
    from mdemi.evaluate import predict_depth
    plan = mf.tile_plan(*img.shape[-2:], TILE, (0, OVERLAP))
    tiles = mf.tile_extract(img, plan)
    preds = []
    for i in range(0, tiles.shape[0], tile_batch):
        chunk = tiles[i:i + tile_batch]
        n = chunk.shape[0]
        if pad and n < tile_batch:
            chunk = torch.cat([chunk] + [chunk[-1:]] * (tile_batch - n))
        preds.append(predict_depth(m, chunk, flip_eval=True)[:n])
    return mf.tile_merge(torch.cat(preds), plan, tuple(img.shape[-2:]))[0]


def test_tiled_predictor_is_extract_predict_merge(model):
    from mdemi.evaluate import TiledPredictor, evaluate_batch
    m, _ = model
    img = _images(2)
    tp = TiledPredictor(m, TILE, OVERLAP, flip_eval=True)
    assert (tp.plan(64, 160).ys, tp.plan(64, 160).xs, tp.plan(64, 160).overlap) == ([0], [0, 64], (0, 32))
    got = tp(img)
    assert got.shape == (2, 1, 64, 160) and tp.coef is None
    want = _chunked_reference(m, img, 4, pad=False)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.isfinite(got).all() and got.min() > 0
    # chunked, and aligned: the same call shape, coefficients kept
    tp2 = TiledPredictor(m, TILE, OVERLAP, align="lstsq", flip_eval=True, tile_batch=2)
    got2 = tp2(img)
    assert got2.shape == got.shape and tp2.coef.shape == (2, 2, 4) and torch.isfinite(got2).all()
    # evaluate_batch takes it where it takes a GraphedPredictor
    eval_opt = {"min_depth_eval": 1e-3, "max_depth_eval": 10.0, "garg_crop": False, "eigen_crop": True}
    gt = torch.rand(2, 1, 64, 160, device=DEV) * 9 + 0.5
    from mdemi.utils.depth_utils import tcompute_errors_gpu
    assert evaluate_batch(tp, img, gt, eval_opt, "KITTI") == tcompute_errors_gpu(got, gt, eval_opt, "KITTI")
    with pytest.raises(ValueError, match="max_depth"):
        TiledPredictor(m, TILE, OVERLAP, align="lstsq_disp")
    with pytest.raises(ValueError, match="align"):
        TiledPredictor(m, TILE, OVERLAP, align="median")
    with pytest.raises(ValueError, match="tile_batch"):
        TiledPredictor(m, TILE, OVERLAP, tile_batch=0)


@pytest.mark.parametrize("tile_batch", [2, 4])
def test_one_captured_graph_serves_every_batch(model, tile_batch):
    """A GraphedPredictor captured at (tile_batch, 3, 64, 96) under a TiledPredictor: 1 image (2
    tiles) and 3 images (6 tiles) replay the one graph and give the bits of the eager chunks; with
    tile_batch 4 the last chunk is short both times and is padded."""
    from mdemi.evaluate import GraphedPredictor, TiledPredictor
    m, _ = model
    gp = GraphedPredictor(m, torch.zeros(tile_batch, 3, *TILE, device=DEV), flip_eval=True)
    tp = TiledPredictor(gp, TILE, OVERLAP)
    assert tp.tile_batch == tile_batch and tp.flip_eval is True
    for n in (1, 3):
        img = _images(n, seed=5 + n)
        got = tp(img)
        assert got.shape == (n, 1, 64, 160)
        assert torch.equal(_bits(got), _bits(_chunked_reference(m, img, tile_batch, pad=True)))
        if tile_batch == 2:  # no padding: the eager TiledPredictor's own chunks
            assert torch.equal(_bits(got), _bits(TiledPredictor(m, TILE, OVERLAP, flip_eval=True, tile_batch=2)(img)))
    wide = _images(1, size=(64, 200), seed=9)  # another image size, the same graph
    assert torch.equal(_bits(tp(wide)), _bits(_chunked_reference(m, wide, tile_batch, pad=True)))
    with pytest.raises(ValueError, match="captured"):
        TiledPredictor(gp, (64, 128), OVERLAP)


def test_tile_of_the_image_size_exports_the_same_files(model, tmp_path):
    from mdemi.evaluate import TiledPredictor
    from mdemi.predict import export_predictions
    m, _ = model
    img = _images(2, size=TILE, seed=3)
    eval_opt = {"min_depth_eval": 1e-3, "max_depth_eval": 10.0, "flip_eval": True}
    paths = ["a/rgb_1.jpg", "b/rgb_2.jpg"]
    plain = export_predictions(m, [(img, paths)], str(tmp_path / "plain"), "NYU", eval_opt)
    tiled = export_predictions(TiledPredictor(m, TILE, (16, 24), flip_eval=True), [(img, paths)],
                               str(tmp_path / "tiled"), "NYU", eval_opt)
    assert len(plain) == len(tiled) == 4
    for p in plain:
        q = p.replace(str(tmp_path / "plain"), str(tmp_path / "tiled"))
        assert q in tiled and open(p, "rb").read() == open(q, "rb").read(), p


def test_predict_cli_with_tiles_and_a_graph(model, tmp_path):
    """python -m mdemi.predict --tile 64 96 --graph (its main(), in process) on a folder that holds
    64x96 and 64x160 frames: every file at its image's size, raw/ = rint(prediction x 1000)."""
    from PIL import Image

    from mdemi.dataset import GpuSampleTransform
    from mdemi.evaluate import TiledPredictor
    from mdemi.predict import main
    m, sd = model
    torch.save({"model": sd}, tmp_path / "w.pth")
    cfg = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
           "eval": {"min_depth_eval": 1e-3, "max_depth_eval": 10.0, "flip_eval": True}}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    rng = np.random.default_rng(11)
    data, lists = tmp_path / "data", tmp_path / "lists" / "NYU"
    (data / "room").mkdir(parents=True)
    lists.mkdir(parents=True)
    frames, lines = [], []
    for i, size in enumerate([(64, 96), (64, 160), (64, 96), (64, 160)]):
        rgb = rng.integers(0, 256, size=size + (3,), dtype=np.uint8)
        Image.fromarray(rgb).save(data / "room" / f"rgb_{i}.png")
        Image.fromarray(rng.integers(500, 9000, size=size, dtype=np.uint16)).save(data / "room" / f"sync_depth_{i}.png")
        frames.append(rgb)
        lines.append(f"/room/rgb_{i}.png /room/sync_depth_{i}.png 518.8579\n")
    (lists / "nyu_test.txt").write_text("".join(lines))
    out = tmp_path / "out"
    written = main(["--config", str(tmp_path / "cfg.json"), "--checkpoint", str(tmp_path / "w.pth"),
                    "--data-path", str(data), "--mode", "test", "--out", str(out), "--batch-size", "1",
                    "--list-root", str(tmp_path / "lists"), "--graph", "--loader-workers", "0", "--tile", "64", "96"])
    assert len(written) == 8
    tp = TiledPredictor(m, TILE, (16, 24), flip_eval=True, tile_batch=1)  # the default overlap: a quarter
    tf = GpuSampleTransform("NYU", "test")
    for i, rgb in enumerate(frames):
        img = tf(torch.from_numpy(rgb[None]), torch.zeros((1,) + rgb.shape[:2], dtype=torch.int16))[0]
        pred = tp(img)[0, 0].cpu().numpy()
        raw = np.asarray(Image.open(out / "raw" / "room" / f"rgb_{i}.png")).astype(np.uint16)
        assert raw.shape == rgb.shape[:2] == pred.shape
        assert np.array_equal(raw, np.rint(pred * np.float32(1000)).astype(np.uint16))
        assert Image.open(out / "vis" / "room" / f"rgb_{i}.png").size == (rgb.shape[1], rgb.shape[0])


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("tile_run")
    (root / "data").mkdir()
    lists = root / "lists" / "NYU"
    lists.mkdir(parents=True)
    (lists / "nyu_train_36k.txt").write_text("".join(_write_frames(str(root / "data"), 1, 0, "train")))
    (lists / "nyu_test.txt").write_text("".join(_write_frames(str(root / "data"), 2, 1, "test")))
    from mdemi.train.builder import build_model
    from mdemi.utils.common_utils import save_checkpoint
    torch.manual_seed(0)
    net = build_model(json.loads(_config(root, "w").read_text()), drop_path=0.0)
    save_checkpoint("w", net, None, 0, 0, 1.0, str(root), model_only=True)
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    yield root
    if env is None:  # common_utils.parse exports the config's gpu_ids
        os.environ.pop("HIP_VISIBLE_DEVICES", None)
    else:
        os.environ["HIP_VISIBLE_DEVICES"] = env


def _test(root, name, *extra, **ev):
    from mdemi import run
    path = _config(root, name)
    if ev:
        cfg = json.loads(path.read_text())
        cfg["eval"].update(ev)
        path.write_text(json.dumps(cfg))
    code = run.main(["--opt", str(path), "--list-root", str(root / "lists"), "--test", "--checkpoint",
                     str(root / "w.pth"), *extra])
    assert code == 0
    rec = json.loads(open(root / name / "log.jsonl").read().splitlines()[-1])
    assert rec["type"] == "test" and all(math.isfinite(rec[k]) for k in METRICS)
    return rec


def test_run_test_logs_the_tiling(workdir):
    """The 480x640 test frames in 256x384 tiles (3 x 2 of them, four at a time)."""
    plain = _test(workdir, "plain")
    assert set(plain) == {"type", "checkpoint", *METRICS}  # without the keys: the record it always was
    rec = _test(workdir, "keys", tile=[256, 384], tile_batch=4)
    assert rec["tile"] == [256, 384] and rec["tile_align"] == "none"
    assert set(rec) == set(plain) | {"tile", "tile_align"}
    assert any(rec[k] != plain[k] for k in METRICS)
    flags = _test(workdir, "flags", "--tile", "256", "384", "--tile-overlap", "64", "96", "--tile-align", "lstsq")
    assert flags["tile"] == [256, 384] and flags["tile_align"] == "lstsq"
    again = _test(workdir, "again", tile=[256, 384], tile_overlap=[64, 96], tile_batch=4)
    assert {k: rec[k] for k in METRICS} == {k: again[k] for k in METRICS}  # the default overlap is a quarter
