"""python -m mdemi.run --test --align end to end on the GPU: the tiny07 NeW-CRFs at 64x96 on two
NYU-format frames, evaluated at the ground truth's 480x640 (75 chunks per image)."""
import json
import math

import pytest
import torch

from test_run_gpu import METRICS, _config, _write_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    import os
    root = tmp_path_factory.mktemp("align_run")
    (root / "data").mkdir()
    lists = root / "lists" / "NYU"
    lists.mkdir(parents=True)
    (lists / "nyu_train_36k.txt").write_text("".join(_write_frames(str(root / "data"), 1, 0, "train")))
    (lists / "nyu_test.txt").write_text("".join(_write_frames(str(root / "data"), 2, 1, "test")))
    from mdemi.train.builder import build_model
    from mdemi.utils.common_utils import save_checkpoint
    torch.manual_seed(0)
    model = build_model(json.loads(_config(root, "w").read_text()), drop_path=0.0)
    save_checkpoint("w", model, None, 0, 0, 1.0, str(root), model_only=True)
    env = os.environ.get("HIP_VISIBLE_DEVICES")
    yield root
    if env is None:  # common_utils.parse exports the config's gpu_ids
        os.environ.pop("HIP_VISIBLE_DEVICES", None)
    else:
        os.environ["HIP_VISIBLE_DEVICES"] = env


def _test(root, name, *extra):
    from mdemi import run
    code = run.main(["--opt", str(_config(root, name)), "--list-root", str(root / "lists"), "--test", "--checkpoint",
                     str(root / "w.pth"), *extra])
    assert code == 0
    rec = json.loads(open(root / name / "log.jsonl").read().splitlines()[-1])
    assert rec["type"] == "test" and all(math.isfinite(rec[k]) for k in METRICS)
    return rec


def test_align_flag_reaches_the_test_record(workdir):
    plain = _test(workdir, "plain")
    assert "align" not in plain
    assert _test(workdir, "none", "--align", "none") == plain
    recs = {mode: _test(workdir, mode, "--align", mode) for mode in ("median", "lstsq", "lstsq_disp")}
    for mode, rec in recs.items():
        assert rec["align"] == mode
        assert any(rec[k] != plain[k] for k in METRICS), mode
    # the prediction is sigmoid x max_depth, inside the evaluated range, so the unaligned clamp is a
    # no-op; least squares in depth minimises each image's squared error before its own clamp,
    # which only moves q towards the in-range ground truth: the mean per-image rmse cannot grow
    assert recs["lstsq"]["rmse"] <= plain["rmse"]
