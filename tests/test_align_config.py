"""eval.align without a GPU: the key and --align are validated before anything starts, the flag
overrides the file, and the numpy align_depth (the CPU counterpart of the GPU path) agrees with
np.median / np.linalg.lstsq and with the fp64 reference of tests/align_ref.py."""
import json
import os

import numpy as np
import pytest

import align_ref as A

CFG = {"model": {"name": "newcrfs", "version": "tiny07"}, "dataset": {"data_type": "NYU"},
       "dataloader": {"batch_size": 2}, "optimizer": {"lr": 1e-4}, "train": {"epoch": 1},
       "loss": {"alpha": 10.0, "beta": 0.15, "per_image": False},
       "eval": {"max_depth_eval": 10, "min_depth_eval": 0.002}}


def _cfg(**ev):
    cfg = json.loads(json.dumps(CFG))
    cfg["eval"].update(ev)
    return cfg


def test_reference_preconditions_hold():
    A.check_preconditions()


def test_eval_align_is_validated():
    from mdemi.train.builder import eval_align
    from mdemi.utils.depth_utils import ALIGN_MODES
    assert ALIGN_MODES == ("none", "median", "lstsq", "lstsq_disp")
    assert eval_align({}) == "none" and eval_align(_cfg()) == "none"
    for mode in ALIGN_MODES:
        assert eval_align(_cfg(align=mode)) == mode
    for bad in ("mean", "Median", "", None, 1, True, ["median"]):
        with pytest.raises(ValueError, match="eval.align"):
            eval_align(_cfg(align=bad))


def test_functional_checks_the_mode_before_anything_runs():
    import torch
    from mdemi import functional as mf
    x = torch.ones(1, 1, 4, 4)  # a CPU tensor: nothing is launched, the check comes first
    for bad in ("none", "mean", 2):
        with pytest.raises(ValueError, match="align mode"):
            mf.depth_align(x, x, (0, 4, 0, 4), 1e-3, 80.0, bad)
        with pytest.raises(ValueError, match="align mode"):
            mf.depth_metrics(x, x, (0, 4, 0, 4), 1e-3, 80.0, align=bad)
    with pytest.raises(ValueError, match="return_aligned"):
        mf.depth_metrics(x, x, (0, 4, 0, 4), 1e-3, 80.0, return_aligned=True)


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


def test_align_flag_overrides_the_file(tmp_path, capsys):
    from mdemi import run
    from mdemi.train.builder import eval_align
    assert run._args(["--opt", "x"]).align is None
    assert run._args(["--opt", "x", "--align", "lstsq"]).align == "lstsq"
    opt = run._override(_cfg(align="median"), run._args(["--opt", "x"]))
    assert eval_align(opt) == "median"
    opt = run._override(_cfg(align="median"), run._args(["--opt", "x", "--align", "lstsq_disp"]))
    assert eval_align(opt) == "lstsq_disp"
    opt = run._override(_cfg(align="median"), run._args(["--opt", "x", "--align", "none"]))
    assert eval_align(opt) == "none"
    opt = run._override({"model": {"name": "newcrfs"}}, run._args(["--opt", "x", "--align", "median"]))
    assert opt["eval"] == {"align": "median"}
    with pytest.raises(SystemExit):  # argparse refuses a bad flag
        run._args(["--opt", "x", "--align", "mean"])
    capsys.readouterr()
    # a bad value in the file is refused before anything else is set up
    cfg = {"gpu_ids": [0], "output_dir": str(tmp_path / "out"), "checkpoint": "", **_cfg(align="mean"),
           "dataset": {"data_type": "NYU", "data_path": str(tmp_path)},
           "dataloader": {"batch_size": 2, "num_workers": 0}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="eval.align"):
        _run_main(["--opt", str(path)])
    with pytest.raises(ValueError, match="eval.align"):
        _run_main(["--opt", str(path), "--test"])


def _masked(shape, b=0):
    pred, gt = A.make_inputs(*shape)
    m = A.valid_mask(gt, A.rect_of(*shape[1:3]))[b]
    return gt[b][m], pred[b][m]


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: f"{s[1]}x{s[2]}")
def test_align_depth_agrees_with_numpy_and_the_reference(shape):
    from mdemi.utils.depth_utils import align_depth
    for b in range(shape[0]):
        g, p = _masked(shape, b)
        q, s, t = align_depth(g, p, "median", A.DMAX)
        assert s == np.median(g.astype(np.float64)) / np.median(p.astype(np.float64)) and t == 0.0
        assert np.array_equal(q, s * p.astype(np.float64))
        q, s, t = align_depth(g, p, "lstsq", A.DMAX)
        want = np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1).astype(np.float64), g.astype(np.float64),
                               rcond=None)[0]
        assert np.allclose([s, t], want, rtol=1e-9, atol=0)
        q, s, t = align_depth(g, p, "lstsq_disp", A.DMAX)
        want = np.linalg.lstsq(np.stack([1.0 / p.astype(np.float64), np.ones(p.size)], 1),
                               1.0 / g.astype(np.float64), rcond=None)[0]
        assert np.allclose([s, t], want, rtol=1e-9, atol=0)
        assert q.min() > 0 and q.max() <= A.DMAX * (1 + 1e-12)
        for mode in A.MODES:  # and with the tests' reference, formula for formula
            q, s, t = align_depth(g, p, mode, A.DMAX)
            ref = A.reference(*shape, mode)
            assert np.allclose([s, t], ref["coef"][b, :2], rtol=1e-12, atol=0)
            assert np.allclose(q, ref["q"][b][ref["mask"][b]], rtol=2e-7)
        q, s, t = align_depth(g, p, "none", A.DMAX)
        assert (s, t) == (1.0, 0.0) and np.array_equal(q, p)


def test_align_depth_recovers_a_known_scale_and_shift():
    from mdemi.utils.depth_utils import align_depth, tcompute_errors
    g, _ = _masked(A.SHAPES[0])
    g = g.astype(np.float64)
    s0, t0 = 2.5, -0.75
    q, s, t = align_depth(g, (g - t0) / s0, "lstsq", A.DMAX)
    assert abs(s - s0) <= 1e-9 * s0 and abs(t - t0) <= 1e-9 * abs(t0)
    q, s, t = align_depth(g, 1.0 / ((1.0 / g - 0.01) / s0), "lstsq_disp", A.DMAX)
    assert abs(s - s0) <= 1e-9 * s0 and abs(t - 0.01) <= 1e-9
    q2, s2, _ = align_depth(g, g / s0, "median", A.DMAX)
    assert abs(s2 - s0) <= 1e-12 * s0
    for aligned in (align_depth(g, (g - t0) / s0, "lstsq", A.DMAX)[0], q, q2):
        m = tcompute_errors(g, aligned)
        assert m["a1"] == m["a2"] == m["a3"] == 1.0
        for k in ("abs_rel", "sq_rel", "rmse", "rmse_log", "log_10"):
            assert m[k] <= 1e-9, (k, m[k])


def test_align_depth_failure_rule():
    from mdemi.utils.depth_utils import align_depth
    g = np.float32([1.0, 2.0, 3.0, 4.0])
    for mode in A.MODES:
        q, s, t = align_depth(g[:0], g[:0], mode, A.DMAX)
        assert (s, t, q.size) == (1.0, 0.0, 0)
        q, s, t = align_depth(g, np.full(4, -1.0, np.float32), mode, A.DMAX)
        assert (s, t) == (1.0, 0.0) and np.array_equal(q, np.full(4, -1.0))
    for mode in ("lstsq", "lstsq_disp"):
        assert align_depth(g, np.full(4, 2.0, np.float32), mode, A.DMAX)[1:] == (1.0, 0.0)
        assert align_depth(g, np.float32([1.0, np.nan, 2.0, 3.0]), mode, A.DMAX)[1:] == (1.0, 0.0)
    with pytest.raises(ValueError, match="mode"):
        align_depth(g, g, "mean", A.DMAX)


def test_valid_records_name_the_alignment(tmp_path):
    """fit() with fakes (in the style of test_run_loop.py): "align" appears in the valid records
    when eval.align is not "none", and only then."""
    from test_run_loop import FakeTelemetry, FakeTrainer
    from mdemi.train.loop import fit
    base = {"dataloader": {"batch_size": 2}, "train": {"print_freq": 2, "valid_freq": 3, "epoch": 1, "num_accum": 1}}
    for ev, want in (({"align": "lstsq"}, "lstsq"), ({"align": "none"}, None), (None, None)):
        out = tmp_path / str(want) / str(ev is None)
        out.mkdir(parents=True)
        opt = dict(base) if ev is None else {**base, "eval": ev}
        code = fit(FakeTrainer(FakeTelemetry()), iter([[("img", "gt")]] * 100), lambda: {"abs_rel": 0.5, "rmse": 1.0},
                   opt, str(out), steps_per_epoch=5, log=lambda s: None)
        assert code == 0
        valid = [r for r in map(json.loads, open(out / "log.jsonl")) if r["type"] == "valid"]
        assert valid and all(r.get("align") == want for r in valid)
        assert all(("align" in r) == (want is not None) for r in valid)
    with pytest.raises(ValueError, match="eval.align"):
        fit(FakeTrainer(FakeTelemetry()), iter([]), lambda: {}, {**base, "eval": {"align": "mean"}}, str(tmp_path),
            steps_per_epoch=5)
