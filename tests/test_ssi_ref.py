"""The fp64 reference of the scale- and shift-invariant loss (tests/ssi_ref.py) against first
principles, without a GPU: central finite differences, numpy's least squares, affine invariance,
the trimming rule on a hand-made case with ties, the skip and NaN rules and both reductions."""
import numpy as np
import pytest

from ssi_ref import SHAPES, SPACES, make_inputs, ssi_image, ssi_ref

MD = 1e-3


@pytest.mark.parametrize("norm", ["none", "gt_var"])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("trim", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("space", SPACES)
def test_gradient_against_central_finite_differences(space, trim, per_image, norm):
    """24 random valid pixels, each moved by +-2^-10 (the step as fp32 took it divides); invalid
    pixels have gradient exactly 0."""
    B, H, W, keep = 2, 9, 11, 0.9
    pred, gt = make_inputs(B, H, W, keep)
    loss, grad, near = ssi_ref(pred, gt, MD, space, trim, norm, per_image)
    assert not near.any() and np.isfinite(loss) and loss > 0
    valid = np.argwhere(gt > MD)
    rng = np.random.default_rng(1)
    h = 2.0 ** -10
    gmax = np.abs(grad).max()
    for b, y, x in valid[rng.choice(len(valid), 24, replace=False)]:
        d, at = [], []
        for sign in (1.0, -1.0):
            q = pred.copy()
            q[b, y, x] += np.float32(sign * h)
            at.append(float(q[b, y, x]))  # the step as fp32 took it
            d.append(ssi_ref(q, gt, MD, space, trim, norm, per_image)[0])
        fd = (d[0] - d[1]) / (at[0] - at[1])
        assert abs(fd - grad[b, y, x]) <= 1e-4 * gmax, (fd, grad[b, y, x], gmax)
    assert (grad[gt <= MD] == 0).all()


@pytest.mark.parametrize("space", SPACES)
def test_scale_and_shift_are_the_least_squares_solution(space):
    pred, gt = make_inputs(*SHAPES[0])
    m = ssi_image(pred[0], gt[0], MD, space)
    A = np.stack([m["x"], np.ones(m["n"])], 1)
    (s, t), *_ = np.linalg.lstsq(A, m["y"], rcond=None)
    assert abs(m["s"] - s) <= 1e-10 * abs(s) and abs(m["t"] - t) <= 1e-10 * max(abs(t), 1.0)
    # the normal equations: sum r = sum r x = 0, which is why A and Bt are defined as 0 at trim 0
    assert abs(m["r"].sum()) <= 1e-9 * np.abs(m["r"]).sum()
    assert abs((m["r"] * m["x"]).sum()) <= 1e-9 * np.abs(m["r"] * m["x"]).sum()
    assert m["A"] == 0.0 and m["Bt"] == 0.0 and m["U"] == m["n"]


@pytest.mark.parametrize("norm", ["none", "gt_var"])
def test_affine_invariance_without_trimming(norm):
    """pred -> a pred + c (depth) and 1/pred -> a/pred + c (disp) leave the loss where it was, up to
    the fp32 rounding of the transformed prediction."""
    pred, gt = make_inputs(*SHAPES[0])
    a, c = 3.0, 0.75
    base = ssi_ref(pred, gt, MD, "depth", 0.0, norm)[0]
    moved = ssi_ref((a * pred.astype(np.float64) + c).astype(np.float32), gt, MD, "depth", 0.0, norm)[0]
    assert abs(moved - base) <= 1e-5 * base
    base = ssi_ref(pred, gt, MD, "disp", 0.0, norm)[0]
    q = (1.0 / (a / pred.astype(np.float64) + c)).astype(np.float32)
    moved = ssi_ref(q, gt, MD, "disp", 0.0, norm)[0]
    assert abs(moved - base) <= 1e-5 * base


def test_trimming_keeps_every_tie_at_tau():
    """x = 1..10 and y = x + off with off orthogonal to 1 and x: s = 1, t = 0 exactly, r = -off.
    |r| has eight equal values at the threshold, all of which stay."""
    x = np.arange(10, dtype=np.float32) + 1
    off = np.array([1, -1, 1, -1, 0, 0, -1, 1, -1, 1], np.float32)  # sum off = sum off x = 0
    assert off.sum() == 0 and (off * x).sum() == 0
    y = x + off
    pred, gt = x.reshape(1, 2, 5), y.reshape(1, 2, 5)
    m = ssi_image(pred[0], gt[0], MD, "depth", trim=0.3)
    assert abs(m["s"] - 1) < 1e-12 and abs(m["t"]) < 1e-12
    # n = 10, u = 10 - floor(0.3 * 10) = 7: the 7th smallest rho is 1, and all eight rho = 1 are kept
    assert m["u"] == 7 and float(m["tau"]) == 1.0 and m["U"] == 10
    off2 = off * np.array([1, 1, 1, 1, 0, 0, 2, 2, 2, 2], np.float32)  # two sizes of residual
    m = ssi_image(x.reshape(2, 5), (x + off2).reshape(2, 5), MD, "depth", trim=0.5)
    u = 10 - 5
    assert m["u"] == u and m["U"] == int((m["rho"] <= m["tau"]).sum()) >= u
    assert (m["rho"][m["k"]] <= m["tau"]).all() and (m["rho"][~m["k"]] > m["tau"]).all()
    assert float(m["tau"]) == float(np.sort(m["rho"])[u - 1])
    # float32(trim) is what multiplies n: 0.45f = 0.44999999 and 0.45f * 20 < 9, so 8 pixels leave, not 9
    x20 = np.arange(20, dtype=np.float32) + 1
    y20 = x20 + np.sin(x20).astype(np.float32)
    assert ssi_image(x20.reshape(4, 5), y20.reshape(4, 5), MD, "depth", trim=0.45)["u"] == 12


@pytest.mark.parametrize("per_image", [False, True])
def test_skip_and_nan_rules_and_both_reductions(per_image):
    pred, gt = make_inputs(*SHAPES[0])
    good = ssi_ref(pred[:1], gt[:1], MD, "depth", 0.2, "gt_var", per_image)
    # image 1: a constant prediction (det == 0 exactly); image 2: no valid pixel
    p, g = pred.copy(), gt.copy()
    p[1] = 2.0
    g[2] = 0.0
    for m, why in ((ssi_image(p[1], g[1]), "det"), (ssi_image(p[2], g[2]), "n")):
        assert m["skip"] and not m["nan"], why
    assert ssi_image(p[1], g[1])["det"] == 0.0
    loss, grad, _ = ssi_ref(p, g, MD, "depth", 0.2, "gt_var", per_image)
    assert loss == good[0] and np.array_equal(grad[0], good[1][0])  # skipped images leave both reductions
    assert not grad[1:].any()
    # a constant ground truth has v == 0 under gt_var only
    g2 = gt.copy()
    g2[1][g2[1] > 0] = 3.0
    assert ssi_image(pred[1], g2[1], norm="gt_var")["skip"] and not ssi_image(pred[1], g2[1])["skip"]
    # nothing usable: 0
    assert ssi_ref(p[1:], g[1:], MD, "depth", 0.0, "none", per_image)[0] == 0.0
    # one image with a single valid pixel: det == 0
    g1 = np.zeros_like(gt[:1])
    g1[0, 5, 5] = 2.0
    assert ssi_image(pred[0], g1[0])["skip"]
    # a NaN prediction on V, and pred == 0 in disp, are not skipped: the loss is NaN
    q = pred.copy()
    y, x = np.argwhere(gt[0] > MD)[0]
    q[0, y, x] = np.nan
    assert np.isnan(ssi_ref(q, gt, MD, "depth", 0.0, "none", per_image)[0])
    q[0, y, x] = 0.0
    assert np.isnan(ssi_ref(q, gt, MD, "disp", 0.2, "none", per_image)[0])
    assert np.isfinite(ssi_ref(q, gt, MD, "depth", 0.2, "none", per_image)[0])
    # the same pixel off V does nothing
    q = pred.copy()
    y, x = np.argwhere(gt[0] <= MD)[0]
    q[0, y, x] = np.nan
    assert ssi_ref(q, gt, MD, "depth", 0.2, "none", per_image)[0] == ssi_ref(pred, gt, MD, "depth", 0.2, "none",
                                                                             per_image)[0]


def test_reductions_differ_as_defined():
    pred, gt = make_inputs(*SHAPES[3])
    ims = [ssi_image(pred[b], gt[b], MD, "disp", 0.2, "gt_var") for b in range(2)]
    per_batch = sum(m["Q"] / m["v"] for m in ims) / (2.0 * sum(m["U"] for m in ims))
    per_img = np.mean([m["Q"] / (2.0 * m["U"] * m["v"]) for m in ims])
    assert abs(ssi_ref(pred, gt, MD, "disp", 0.2, "gt_var", False)[0] - per_batch) <= 1e-15 * per_batch
    assert abs(ssi_ref(pred, gt, MD, "disp", 0.2, "gt_var", True)[0] - per_img) <= 1e-15 * per_img


@pytest.mark.parametrize("trim", [0.2, 0.5])
@pytest.mark.parametrize("space", SPACES)
def test_no_near_tau_pixel_on_the_shared_inputs(space, trim):
    """The GPU test's cap (near <= 1 % of the valid pixels) is met by the reference alone."""
    for shape in SHAPES:
        pred, gt = make_inputs(*shape)
        near = ssi_ref(pred, gt, MD, space, trim)[2]
        assert near.sum() <= 0.01 * (gt > MD).sum(), (shape, int(near.sum()))
