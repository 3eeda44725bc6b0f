"""python -m mdemi.run --test --boundary end to end on the GPU: the tiny07 NeW-CRFs at 64x96 on two
NYU-format frames, evaluated at the ground truth's 480x640.  test_run_gpu's frames are smooth (no
depth ratio of neighbours reaches 1.05), so the first test frame gets two boxes of other depths
painted into its ground truth; the second stays smooth and so has no boundary score."""
import json
import math

import numpy as np
import pytest
import torch

from test_run_gpu import METRICS, _config, _write_frames

pytestmark = pytest.mark.gpu
KEYS = ("boundary_f1", "boundary_precision", "boundary_recall")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    import os
    from PIL import Image
    root = tmp_path_factory.mktemp("boundary_run")
    (root / "data").mkdir()
    lists = root / "lists" / "NYU"
    lists.mkdir(parents=True)
    (lists / "nyu_train_36k.txt").write_text("".join(_write_frames(str(root / "data"), 1, 0, "train")))
    (lists / "nyu_test.txt").write_text("".join(_write_frames(str(root / "data"), 2, 1, "test")))
    path = root / "data" / "test_depth_0000.png"
    dep = np.array(Image.open(path))
    assert dep.dtype == np.uint16 and dep.shape == (480, 640)
    dep[100:220, 150:300] = 1500  # millimetres; inside NYU's eigen crop
    dep[260:400, 350:560] = 8000
    Image.fromarray(dep).save(path)
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


def _test(root, name, *extra, **ev):
    from mdemi import run
    cfg_path = _config(root, name)
    if ev:
        cfg = json.loads(cfg_path.read_text())
        cfg["eval"].update(ev)
        cfg_path.write_text(json.dumps(cfg))
    code = run.main(["--opt", str(cfg_path), "--list-root", str(root / "lists"), "--test", "--checkpoint",
                     str(root / "w.pth"), *extra])
    assert code == 0
    rec = json.loads(open(root / name / "log.jsonl").read().splitlines()[-1])
    assert rec["type"] == "test" and all(math.isfinite(rec[k]) for k in METRICS)
    return rec


def test_boundary_flag_reaches_the_test_record(workdir):
    plain = _test(workdir, "plain")
    assert not any(k.startswith("boundary") for k in plain)
    assert _test(workdir, "off", boundary=False) == plain
    rec = _test(workdir, "on", "--boundary")
    for k in KEYS:
        assert math.isfinite(rec[k]) and 0.0 <= rec[k] <= 1.0, (k, rec[k])
    assert rec["boundary_images"] == 1 and isinstance(rec["boundary_images"], int)  # the smooth frame has no score
    assert rec["boundary"] == [1.05, 1.25, 10]
    assert {k: rec[k] for k in plain} == plain  # the nine metrics are unchanged
    assert _test(workdir, "cfg", boundary=True) == rec
    other = _test(workdir, "n3", boundary={"t_min": 1.1, "t_max": 1.5, "n": 3})
    assert other["boundary"] == [1.1, 1.5, 3] and other["boundary_images"] == 1
    both = _test(workdir, "both", "--boundary", "--align", "lstsq")
    assert both["align"] == "lstsq" and both["boundary"] == [1.05, 1.25, 10] and both["boundary_images"] == 1
    assert all(math.isfinite(both[k]) and 0.0 <= both[k] <= 1.0 for k in KEYS)
    aligned = _test(workdir, "aligned", "--align", "lstsq")
    assert {k: both[k] for k in aligned} == aligned
