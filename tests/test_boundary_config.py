"""eval.boundary without a GPU: the key and --boundary are validated before anything starts, and
evaluate()'s reduction (MetricMeans) leaves an image without a boundary score out of the boundary
means and in the nine."""
import json
import os

import pytest

CFG = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
       "dataloader": {"batch_size": 2}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1},
       "loss": {"alpha": 10.0, "beta": 0.15, "per_image": False},
       "eval": {"max_depth_eval": 10, "min_depth_eval": 0.002}}
NINE = ("a1", "a2", "a3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log_10")


def _cfg(**ev):
    cfg = json.loads(json.dumps(CFG))
    cfg["eval"].update(ev)
    return cfg


def test_eval_boundary_is_validated():
    from mdemi.train.builder import eval_boundary
    from mdemi.utils.depth_utils import METRICS
    assert METRICS == NINE  # the nine stay the nine
    assert eval_boundary({}) is None and eval_boundary(_cfg()) is None
    assert eval_boundary(_cfg(boundary=False)) is None and eval_boundary(_cfg(boundary=None)) is None
    assert eval_boundary(_cfg(boundary=True)) == (1.05, 1.25, 10)
    assert eval_boundary(_cfg(boundary={})) == (1.05, 1.25, 10)
    assert eval_boundary(_cfg(boundary={"t_min": 1.1, "t_max": 1.5, "n": 4})) == (1.1, 1.5, 4)
    assert eval_boundary(_cfg(boundary={"n": 16})) == (1.05, 1.25, 16)
    assert eval_boundary(_cfg(boundary={"t_min": 1.25, "n": 1})) == (1.25, 1.25, 1)
    assert eval_boundary(_cfg(boundary={"t_min": 2, "t_max": 3})) == (2.0, 3.0, 10)
    bad = [({"tmin": 1.1}, "eval.boundary.tmin"), ({"t_min": 1.1, "levels": 3}, "eval.boundary.levels"),
           ({"t_min": 1.0}, "eval.boundary.t_min"), ({"t_min": 0.5}, "eval.boundary.t_min"),
           ({"t_min": True}, "eval.boundary.t_min"), ({"t_min": "1.1"}, "eval.boundary.t_min"),
           ({"t_min": float("nan")}, "eval.boundary.t_min"),
           ({"t_min": 1.3}, "eval.boundary.t_max"), ({"t_max": 1.01}, "eval.boundary.t_max"),
           ({"t_max": True}, "eval.boundary.t_max"), ({"t_max": None}, "eval.boundary.t_max"),
           ({"t_max": float("inf")}, "eval.boundary.t_max"),
           ({"n": 0}, "eval.boundary.n"), ({"n": 17}, "eval.boundary.n"), ({"n": -1}, "eval.boundary.n"),
           ({"n": True}, "eval.boundary.n"), ({"n": 4.0}, "eval.boundary.n"), ({"n": "4"}, "eval.boundary.n")]
    for spec, key in bad:
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            eval_boundary(_cfg(boundary=spec))
    for spec in (1, "true", [1.05, 1.25, 10], 0):
        with pytest.raises(ValueError, match=r"eval\.boundary"):
            eval_boundary(_cfg(boundary=spec))


def _run_main(argv):
    from mdemi import run
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    try:
        return run.main(argv)
    finally:  # parse() exports the config's gpu_ids
        if env is None:
            os.environ.pop("HIP_VISIBLE_DEVICES", None)
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = env


def test_boundary_flag_reaches_opt(tmp_path, capsys):
    from mdemi import run
    from mdemi.train.builder import eval_boundary
    assert run._args(["--opt", "x"]).boundary is False
    assert run._args(["--opt", "x", "--boundary"]).boundary is True
    opt = run._override(_cfg(), run._args(["--opt", "x"]))
    assert "boundary" not in opt["eval"] and eval_boundary(opt) is None
    opt = run._override(_cfg(), run._args(["--opt", "x", "--boundary"]))
    assert opt["eval"]["boundary"] is True and eval_boundary(opt) == (1.05, 1.25, 10)
    opt = run._override(_cfg(boundary=False), run._args(["--opt", "x", "--boundary"]))
    assert eval_boundary(opt) == (1.05, 1.25, 10)
    opt = run._override({"model": {"name": "newcrfs"}}, run._args(["--opt", "x", "--boundary"]))
    assert opt["eval"] == {"boundary": True}
    # the file's own thresholds stand when the flag is absent
    opt = run._override(_cfg(boundary={"n": 3}), run._args(["--opt", "x"]))
    assert eval_boundary(opt) == (1.05, 1.25, 3)
    capsys.readouterr()
    # a bad value in the file is refused before anything else is set up
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "", **_cfg(boundary={"n": 17}),
           "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match=r"eval\.boundary\.n"):
        _run_main(["--opt", str(path)])
    with pytest.raises(ValueError, match=r"eval\.boundary\.n"):
        _run_main(["--opt", str(path), "--test"])


def test_functional_checks_its_arguments_before_anything_runs():
    import numpy as np
    import torch
    from mdemi import functional as mf
    x = torch.ones(1, 1, 4, 4)  # a CPU tensor: nothing is launched, the checks come first
    with pytest.raises(ValueError, match="thresholds"):
        mf.depth_boundary(x, x, (0, 4, 0, 4), 1e-3, 10.0, thresholds=np.float32([1.0]))
    with pytest.raises(ValueError, match="thresholds"):
        mf.depth_boundary(x, x, (0, 4, 0, 4), 1e-3, 10.0, thresholds=[1.1, 1.2])
    with pytest.raises(ValueError, match="align mode"):
        mf.depth_boundary(x, x, (0, 4, 0, 4), 1e-3, 10.0, align="none")
    with pytest.raises(ValueError, match="coef"):
        mf.depth_boundary(x, x, (0, 4, 0, 4), 1e-3, 10.0, coef=torch.zeros(1, 4, dtype=torch.float64))


def _rows():
    """Three images' dicts as tcompute_errors_gpu makes them; the second has no boundary score."""
    rows = [{k: 0.1 * (i + 1) + 0.01 * j for j, k in enumerate(NINE)} for i in range(3)]
    rows[0].update(boundary_f1=0.5, boundary_precision=0.4, boundary_recall=0.75)
    rows[2].update(boundary_f1=0.25, boundary_precision=0.5, boundary_recall=0.125)
    return rows


def test_metric_means_keeps_the_unscored_image_in_the_nine_only():
    from mdemi.evaluate import MetricMeans
    for weight_by_count in (False, True):
        plain = MetricMeans()
        for r in _rows():
            plain.update({k: r[k] for k in NINE})
        want = plain.result(weight_by_count)
        assert tuple(want) == NINE
        m = MetricMeans(boundary=True)
        for r in _rows():
            m.update(r)
        got = m.result(weight_by_count)
        assert tuple(got) == NINE + ("boundary_f1", "boundary_precision", "boundary_recall", "boundary_images")
        assert {k: got[k] for k in NINE} == want  # the same bits in the nine
        for j, k in enumerate(NINE):
            assert abs(got[k] - (0.2 + 0.01 * j)) < 1e-12  # all three images
        assert got["boundary_images"] == 2 and isinstance(got["boundary_images"], int)
        assert got["boundary_f1"] == (0.5 + 0.25) / 2  # the two that have a score: not (0.5 + 0 + 0.25) / 3
        assert got["boundary_precision"] == (0.4 + 0.5) / 2 and got["boundary_recall"] == (0.75 + 0.125) / 2
        # the unscored image first: the running averages are keyed by the first dict they see
        m = MetricMeans(boundary=True)
        for r in (_rows()[1], _rows()[0], _rows()[2]):
            m.update(r)
        assert m.result(weight_by_count)["boundary_f1"] == (0.5 + 0.25) / 2
        # no image with a score: the three keys are absent, the count is 0
        m = MetricMeans(boundary=True)
        m.update(_rows()[1])
        got = m.result(weight_by_count)
        assert tuple(got) == NINE + ("boundary_images",) and got["boundary_images"] == 0


class _FakeModel:
    training = True

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode


def test_evaluate_reduces_fake_rows(monkeypatch):
    """evaluate() with a fake model and fake per-image dicts: eval.boundary switches the boundary
    means on, and without the key the result is the nine alone."""
    from mdemi import evaluate as E
    rows = _rows()
    monkeypatch.setattr(E, "evaluate_batch", lambda model, img, gt, eval_opt, data_type: [rows[img]])
    batches = [(0, None), (1, None), (2, None)]
    model = _FakeModel()
    got = E.evaluate(model, batches, {"boundary": True}, "NYU", weight_by_count=True)
    assert model.training is True
    assert got["boundary_images"] == 2 and got["boundary_f1"] == 0.375
    assert abs(got["abs_rel"] - (0.2 + 0.03)) < 1e-12
    nine = [{k: r[k] for k in NINE} for r in rows]
    monkeypatch.setattr(E, "evaluate_batch", lambda model, img, gt, eval_opt, data_type: [nine[img]])
    for ev in ({}, {"boundary": False}):
        plain = E.evaluate(model, batches, ev, "NYU", weight_by_count=True)
        assert tuple(plain) == NINE and plain == {k: got[k] for k in NINE}
    with pytest.raises(ValueError, match=r"eval\.boundary\.n"):
        E.evaluate(model, batches, {"boundary": {"n": 0}}, "NYU")


def test_valid_records_carry_the_boundary_scores(tmp_path):
    """fit() with fakes (in the style of test_run_loop.py): under eval.boundary the valid records
    carry what validate() returned, "boundary_images" as an integer and "boundary": [t_min, t_max,
    n]; best.pth is still chosen on abs_rel; without the key the records are as before."""
    from test_run_loop import FakeTelemetry, FakeTrainer
    from mdemi.train.loop import fit
    base = {"dataloader": {"batch_size": 2}, "train": {"print_freq": 2, "valid_freq": 3, "epoch": 1, "num_accum": 1}}
    scored = {"abs_rel": 0.5, "rmse": 1.0, "boundary_f1": 0.25, "boundary_precision": 0.5, "boundary_recall": 0.125,
              "boundary_images": 2.0}
    for ev, metrics, want in (({"boundary": True}, scored, [1.05, 1.25, 10]),
                              ({"boundary": {"n": 3}}, {"abs_rel": 0.5, "rmse": 1.0, "boundary_images": 0},
                               [1.05, 1.25, 3]),
                              ({"boundary": False}, {"abs_rel": 0.5, "rmse": 1.0}, None),
                              (None, {"abs_rel": 0.5, "rmse": 1.0}, None)):
        out = tmp_path / f"{want}-{ev is None}"
        out.mkdir(parents=True)
        opt = dict(base) if ev is None else {**base, "eval": ev}
        code = fit(FakeTrainer(FakeTelemetry()), iter([[("img", "gt")]] * 100), lambda: dict(metrics), opt, str(out),
                   steps_per_epoch=5, log=lambda s: None)
        assert code == 0
        valid = [r for r in map(json.loads, open(out / "log.jsonl")) if r["type"] == "valid"]
        assert valid and valid[0]["best"] is True
        for r in valid:
            assert r.get("boundary") == want and ("boundary" in r) == (want is not None)
            assert ("boundary_images" in r) == (want is not None)
            if want is not None:
                assert isinstance(r["boundary_images"], int) and r["boundary_images"] == int(metrics["boundary_images"])
            assert ("boundary_f1" in r) == ("boundary_f1" in metrics)
            assert r["abs_rel"] == 0.5
    with pytest.raises(ValueError, match=r"eval\.boundary\.t_min"):
        fit(FakeTrainer(FakeTelemetry()), iter([]), lambda: {}, {**base, "eval": {"boundary": {"t_min": 1}}},
            str(tmp_path), steps_per_epoch=5)
