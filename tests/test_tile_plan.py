"""Tiled inference without a GPU: the plan's properties over a sweep of sizes, the numpy
merge_tiles (the CPU counterpart of the GPU merge) against the independent fp64 reference of
tests/tile_ref.py, the failure rule, and the validation of the four eval.tile* keys and their flags."""
import json

import numpy as np
import pytest

import tile_ref as R

CASES = [((37, 53), (16, 24), (5, 7)), ((40, 56), (24, 32), (8, 8)), ((20, 200), (32, 64), (0, 16)),
         ((24, 32), (24, 32), (0, 0))]
IDS = ["37x53", "40x56", "20x200", "24x32"]


def test_plan_properties_over_a_sweep():
    from mdemi.utils.depth_utils import tile_plan
    seen_multi = 0
    for H in range(1, 81):
        for t in (1, 2, 3, 7, 16, 24, 80, 100):
            for o in (0, 1, 2, 5, 15, 23):
                tc = min(t, H)
                if o >= tc:
                    with pytest.raises(ValueError, match="overlap"):
                        tile_plan(H, 9, (t, 4), (o, 0))
                    continue
                n = 1 if H == tc else -(-(H - o) // (tc - o))
                if n > 32:
                    with pytest.raises(ValueError, match="at most 32"):
                        tile_plan(H, 9, (t, 4), (o, 0))
                    continue
                p = tile_plan(H, 9, (t, 4), (o, 0))
                q = tile_plan(9, H, (4, t), (0, o))  # the same rule on the other axis
                assert p.ys == q.xs and p.tile[0] == q.tile[1] == tc and p.size == (H, 9) and p.overlap == (o, 0)
                ys = p.ys
                assert (tc, ys) == R.axis_origins(H, t, o) and len(ys) == n
                assert ys[0] == 0 and ys[-1] == H - tc and all(0 <= y <= H - tc for y in ys)
                assert all(b > a for a, b in zip(ys, ys[1:]))
                assert all(a + tc - b >= o for a, b in zip(ys, ys[1:])), (H, t, o, ys)  # neighbours' overlap
                covered = np.zeros(H, bool)
                for y in ys:
                    covered[y:y + tc] = True
                assert covered.all()
                if H <= t:
                    assert ys == [0]
                seen_multi += n > 2
    assert seen_multi > 100


def test_plan_refusals():
    from mdemi.utils.depth_utils import tile_plan
    assert tile_plan(64, 160, (64, 96), 32).xs == [0, 64]
    assert tile_plan(37, 53, [16, 24], [5, 7])[:3] == ([0, 10, 21], [0, 14, 29], (16, 24))
    for bad in ((0, 4), (4,), (4, 4, 4), "44", 4.0, (4.0, 4), (True, 4), None):
        with pytest.raises(ValueError, match="tile"):
            tile_plan(8, 8, bad)
    for bad in (-1, (0, -1), (1, 2, 3), 1.5, None, (False, 0)):
        with pytest.raises(ValueError, match="overlap"):
            tile_plan(8, 8, (4, 4), bad)
    with pytest.raises(ValueError, match="overlap"):
        tile_plan(8, 8, (4, 4), 4)
    with pytest.raises(ValueError, match="overlap"):
        tile_plan(3, 8, (4, 4), 3)  # the tile is clipped to 3 rows first
    with pytest.raises(ValueError, match="image size"):
        tile_plan(0, 8, (4, 4))
    with pytest.raises(ValueError, match="at most 32"):
        tile_plan(8, 100, (4, 4), 2)


def test_weights_are_the_ramp():
    from mdemi.utils.depth_utils import tile_plan, tile_weights
    wy, wx = tile_weights(tile_plan(37, 53, (16, 24), (5, 7)))
    assert wy.dtype == np.float64 and np.array_equal(wy, R.ramp(16, 5)) and np.array_equal(wx, R.ramp(24, 7))
    assert wy.tolist() == [1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 5, 5, 4, 3, 2, 1]
    wy, wx = tile_weights(tile_plan(20, 200, (32, 64), (0, 16)))
    assert wy.tolist() == [1.0] * 20 and wx.min() == 1 and wx.max() == 16


def _merge_both(tiles, size, tile, overlap, align, max_depth=None):
    from mdemi.utils.depth_utils import merge_tiles, tile_plan
    got, coef = merge_tiles(tiles, tile_plan(*size, tile, overlap), align, max_depth)
    want, wcoef, blend = R.merge(tiles, size, tile, overlap, align, max_depth)
    assert got.dtype == np.float32 and got.shape == (want.shape[0], 1) + size
    return got[:, 0], coef, want, wcoef, blend


@pytest.mark.parametrize("size,tile,overlap", CASES, ids=IDS)
def test_constant_tiles_give_the_constant(size, tile, overlap):
    T = len(R.axis_origins(size[0], tile[0], overlap[0])[1]) * len(R.axis_origins(size[1], tile[1], overlap[1])[1])
    th, tw = min(tile[0], size[0]), min(tile[1], size[1])
    tiles = np.full((2 * T, th, tw), 3.7, np.float32)
    got, coef, want, _, _ = _merge_both(tiles, size, tile, overlap, "none")
    assert coef is None and np.array_equal(got, want) and np.all(got == np.float32(3.7))
    # (B*T,1,th,tw) is taken too
    from mdemi.utils.depth_utils import merge_tiles, tile_plan
    assert np.array_equal(merge_tiles(tiles[:, None], tile_plan(*size, tile, overlap))[0][:, 0], got)


@pytest.mark.parametrize("size,tile,overlap", CASES, ids=IDS)
def test_blend_agrees_with_the_reference(size, tile, overlap):
    _, tiles = R.recoverable(size, tile, overlap, "none", seed=3, noise=0.05)
    got, _, want, _, _ = _merge_both(tiles, size, tile, overlap, "none")
    assert np.array_equal(got, want)  # the same fp64 operations in the same order
    if overlap == (0, 0) or tiles.shape[0] == 2:  # a pixel under one tile takes that tile's value
        assert np.array_equal(got, tiles.reshape(got.shape))


@pytest.mark.parametrize("align", ["lstsq", "lstsq_disp"])
@pytest.mark.parametrize("size,tile,overlap", [c for c in CASES if c[2] != (0, 0)][:2] + [((20, 200), (32, 64), (3, 16))],
                         ids=["37x53", "40x56", "20x200"])
def test_known_transforms_are_undone(size, tile, overlap, align):
    """Tiles cut from one map, each given a scale in [0.5, 2] and a shift within 10 % of the range,
    come back in tile 0's frame.  The tiles are fp32, so each carries a relative rounding error of
    2^-24 that the fits (over hundreds of pixels) pass on at most T times along the chain: 1e-5
    relative is ~170 x 2^-24."""
    D, tiles = R.recoverable(size, tile, overlap, align, seed=5)
    got, coef, want, wcoef, blend = _merge_both(tiles, size, tile, overlap, align, R.MAX_DEPTH)
    T = coef.shape[1]
    assert np.array_equal(coef[:, 0], np.tile([1.0, 0.0, 0.0, 0.0], (2, 1)))
    assert np.array_equal(coef[..., 2:], wcoef[..., 2:]) and np.all(coef[..., 3] == 0) and np.all(coef[:, 1:, 2] >= 2)
    assert np.allclose(coef[..., :2], wcoef[..., :2], rtol=1e-12 * T, atol=1e-13)
    assert R.ulp_diff(got, want).max() <= 1
    err = np.abs(blend - D).max() / D.max()
    print(f"{align} {size}: T={T}, recovery max|err|/max D = {err:.2e}")
    assert err <= 1e-5
    assert np.abs(got - D).max() / D.max() <= 1e-5 + 2.0 ** -24


def test_failure_rule():
    from mdemi.utils.depth_utils import merge_tiles, tile_plan
    size, tile, overlap = (16, 40), (16, 24), (0, 8)  # two tiles sharing columns 16..23
    plan = tile_plan(*size, tile, overlap)
    assert plan.xs == [0, 16]
    D, tiles = R.recoverable(size, tile, overlap, "lstsq", B=1, seed=1)
    for align in ("lstsq", "lstsq_disp"):
        # an overlap that is all NaN (in the anchor): n = 0
        t = tiles.copy()
        t[0, :, 16:] = np.nan
        # a constant tile: det = 0
        c = tiles.copy()
        c[1] = 2.0
        # a negative fitted scale: the second tile descends where the first ascends
        n = tiles.copy()
        n[0] = 2.0 + np.arange(24, dtype=np.float32)[None, :] / 8
        n[1] = (6.0 - np.arange(24, dtype=np.float32)[None, :] / 8) if align == "lstsq" else n[0, :, ::-1]
        for name, x, cnt in (("nan", t, 0.0), ("const", c, 128.0), ("neg", n, 128.0)):
            got, coef = merge_tiles(x, plan, align, R.MAX_DEPTH)
            want, wcoef, _ = R.merge(x, size, tile, overlap, align, R.MAX_DEPTH)
            assert coef[0, 1].tolist() == [1.0, 0.0, cnt, 1.0] == wcoef[0, 1].tolist(), (align, name, coef, wcoef)
            assert np.array_equal(got[:, 0], want, equal_nan=True)
            if name == "nan":
                assert np.isnan(got[0, 0, :, 16:24]).all() and np.isfinite(got[0, 0, :, :16]).all()
                assert np.isfinite(got[0, 0, :, 24:]).all()
            # a failed tile is blended as it is
            plain = merge_tiles(1.0 / x if align == "lstsq_disp" else x, plan)[0]
            if align == "lstsq_disp":
                plain = 1.0 / np.maximum(plain.astype(np.float64), 1.0 / R.MAX_DEPTH)
            assert np.allclose(got, plain, rtol=1e-6, equal_nan=True)
    # one pair is not a fit either
    plan1 = tile_plan(1, 7, (1, 4), (0, 1))
    got, coef = merge_tiles(np.float32([[[1, 2, 3, 4]], [[5, 6, 7, 8]]]), plan1, "lstsq")
    assert coef[0, 1].tolist() == [1.0, 0.0, 1.0, 1.0]


def test_merge_refusals():
    from mdemi.utils.depth_utils import merge_tiles, tile_plan
    plan = tile_plan(20, 200, (32, 64), (0, 16))  # one tile along y: its zero overlap is fine
    tiles = np.ones((4, 20, 64), np.float32)
    assert merge_tiles(tiles, plan, "lstsq")[1].shape == (1, 4, 4)
    gap = tile_plan(40, 200, (32, 64), (0, 16))
    with pytest.raises(ValueError, match="overlap of 0"):
        merge_tiles(np.ones((8, 32, 64), np.float32), gap, "lstsq")
    assert merge_tiles(np.ones((8, 32, 64), np.float32), gap, "none")[1] is None
    with pytest.raises(ValueError, match="max_depth"):
        merge_tiles(tiles, plan, "lstsq_disp")
    with pytest.raises(ValueError, match="align"):
        merge_tiles(tiles, plan, "median")
    with pytest.raises(ValueError, match="tiles must be"):
        merge_tiles(tiles[:3], plan)
    with pytest.raises(ValueError, match="tiles must be"):
        merge_tiles(tiles[:, :19], plan)


def test_functional_refuses_before_anything_runs():
    import torch
    from mdemi import functional as mf
    plan = mf.tile_plan(40, 56, (24, 32), 8)
    assert plan == mf.tile_plan(40, 56, [24, 32], [8, 8]) and (plan.ys, plan.xs) == ([0, 16], [0, 24])
    with pytest.raises(ValueError, match="GPU only"):
        mf.tile_extract(torch.ones(1, 3, 40, 56), plan)
    with pytest.raises(ValueError, match="GPU only"):
        mf.tile_merge(torch.ones(4, 1, 24, 32), plan, (40, 56))
    with pytest.raises(ValueError, match="align"):
        mf.tile_merge(torch.ones(4, 1, 24, 32), plan, (40, 56), align="median")
    with pytest.raises(ValueError, match="max_depth"):
        mf.tile_merge(torch.ones(4, 1, 24, 32), plan, (40, 56), align="lstsq_disp")
    with pytest.raises(ValueError, match="overlap of 0"):
        mf.tile_merge(torch.ones(4, 1, 24, 32), mf.tile_plan(40, 56, (24, 32), (8, 0)), (40, 56), align="lstsq")


CFG = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
       "dataloader": {"batch_size": 2}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1},
       "eval": {"max_depth_eval": 10, "min_depth_eval": 0.002}}


def _cfg(**ev):
    cfg = json.loads(json.dumps(CFG))
    cfg["eval"].update(ev)
    return cfg


def test_eval_tile_keys_are_validated():
    from mdemi.train.builder import eval_tile
    assert eval_tile({}) is None and eval_tile(_cfg()) is None
    assert eval_tile(_cfg(tile=[352, 704])) == {"tile": (352, 704), "overlap": (88, 176), "align": "none",
                                                "tile_batch": None, "max_depth": 10}
    got = eval_tile(_cfg(tile=[64, 96], tile_overlap=32, tile_align="lstsq_disp", tile_batch=2))
    assert got == {"tile": (64, 96), "overlap": (32, 32), "align": "lstsq_disp", "tile_batch": 2, "max_depth": 10}
    assert eval_tile(_cfg(tile=[64, 96], tile_overlap=[0, 16]))["overlap"] == (0, 16)
    for bad in (64, [64], [64, 96, 3], [0, 96], [64.0, 96], "64x96", [True, 96], {"h": 64}):
        with pytest.raises(ValueError, match="eval.tile"):
            eval_tile(_cfg(tile=bad))
    for bad in (-1, [8], [8, -1], 64, [8, 96], 1.5, "8", None, True):
        with pytest.raises(ValueError, match="eval.tile_overlap"):
            eval_tile(_cfg(tile=[64, 96], tile_overlap=bad))
    for bad in ("median", "Lstsq", "", None, 2, ["lstsq"]):
        with pytest.raises(ValueError, match="eval.tile_align"):
            eval_tile(_cfg(tile=[64, 96], tile_align=bad))
    for bad in (0, -2, 1.0, "2", True, [2]):
        with pytest.raises(ValueError, match="eval.tile_batch"):
            eval_tile(_cfg(tile=[64, 96], tile_batch=bad))
    for key, v in (("tile_overlap", 8), ("tile_align", "lstsq"), ("tile_batch", 2)):
        with pytest.raises(ValueError, match="eval.tile is not"):
            eval_tile(_cfg(**{key: v}))
    cfg = _cfg(tile=[64, 96], tile_align="lstsq_disp")
    del cfg["eval"]["max_depth_eval"]
    with pytest.raises(ValueError, match="max_depth_eval"):
        eval_tile(cfg)


def test_tile_flags_override_the_file(tmp_path, capsys):
    import os
    from mdemi import run
    from mdemi.train.builder import eval_tile
    a = run._args(["--opt", "x"])
    assert a.tile is None and a.tile_overlap is None and a.tile_align is None
    assert "tile" not in run._override(_cfg(), a)["eval"]
    opt = run._override(_cfg(tile=[32, 32], tile_align="lstsq"), run._args(["--opt", "x", "--tile", "64", "96"]))
    assert eval_tile(opt)["tile"] == (64, 96) and eval_tile(opt)["align"] == "lstsq"
    opt = run._override(_cfg(), run._args(["--opt", "x", "--tile", "64", "96", "--tile-overlap", "8", "--tile-align",
                                          "lstsq_disp"]))
    assert opt["eval"]["tile_overlap"] == 8 and eval_tile(opt)["overlap"] == (8, 8)
    assert eval_tile(opt)["align"] == "lstsq_disp"
    opt = run._override(_cfg(), run._args(["--opt", "x", "--tile", "64", "96", "--tile-overlap", "8", "16"]))
    assert eval_tile(opt)["overlap"] == (8, 16)
    with pytest.raises(SystemExit):
        run._override(_cfg(), run._args(["--opt", "x", "--tile", "64", "96", "--tile-overlap", "1", "2", "3"]))
    with pytest.raises(SystemExit):
        run._args(["--opt", "x", "--tile", "64"])
    with pytest.raises(SystemExit):
        run._args(["--opt", "x", "--tile-align", "median"])
    capsys.readouterr()
    # a bad value is refused before anything else is set up, by mdemi.run and by mdemi.predict
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "", **_cfg(tile=[64, 96], tile_overlap=96),
           "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    try:
        for extra in ([], ["--test"]):
            with pytest.raises(ValueError, match="eval.tile_overlap"):
                run.main(["--opt", str(path), *extra])
        with pytest.raises(ValueError, match="eval.tile_overlap"):
            run.main(["--opt", str(path), "--tile-overlap", "8", "200"])
    finally:  # parse() exports the config's gpu_ids
        if env is None:
            os.environ.pop("HIP_VISIBLE_DEVICES", None)
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = env
    from mdemi import predict
    with pytest.raises(ValueError, match="eval.tile_overlap"):
        predict.main(["--config", str(path), "--checkpoint", "none.pth", "--data-path", str(tmp_path), "--out",
                      str(tmp_path / "o")])


def test_valid_records_name_the_tiling(tmp_path):
    """fit() with fakes (in the style of test_run_loop.py): "tile" and "tile_align" appear in the
    valid records when eval.tile is set, and only then."""
    from test_run_loop import FakeTelemetry, FakeTrainer
    from mdemi.train.loop import fit
    base = {"dataloader": {"batch_size": 2}, "train": {"print_freq": 2, "valid_freq": 3, "epoch": 1, "num_accum": 1}}
    for i, (ev, want) in enumerate((({"tile": [64, 96], "tile_align": "lstsq", "max_depth_eval": 10}, "lstsq"),
                                    ({"tile": [64, 96]}, "none"), ({}, None), (None, None))):
        out = tmp_path / str(i)
        out.mkdir()
        opt = dict(base) if ev is None else {**base, "eval": ev}
        code = fit(FakeTrainer(FakeTelemetry()), iter([[("img", "gt")]] * 100), lambda: {"abs_rel": 0.5, "rmse": 1.0},
                   opt, str(out), steps_per_epoch=5, log=lambda s: None)
        assert code == 0
        valid = [r for r in map(json.loads, open(out / "log.jsonl")) if r["type"] == "valid"]
        assert valid
        for r in valid:
            if want is None:
                assert "tile" not in r and "tile_align" not in r
            else:
                assert r["tile"] == [64, 96] and r["tile_align"] == want
    with pytest.raises(ValueError, match="eval.tile"):
        fit(FakeTrainer(FakeTelemetry()), iter([]), lambda: {}, {**base, "eval": {"tile": [64]}}, str(tmp_path),
            steps_per_epoch=5)
