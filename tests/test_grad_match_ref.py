"""The fp64 reference of the gradient-matching loss (tests/grad_match_ref.py) checked on its own,
without a GPU: its gradient against central differences, its scale invariance, a case worked by
hand and the two normalisers."""
import numpy as np

from grad_match_ref import SHAPES, grad_match_ref, grad_match_sums, make_inputs


def _small(seed=3, B=2, H=9, W=11):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 9.5, (B, H, W))
    gt[rng.uniform(size=gt.shape) < 0.2] = 0.0
    pred = rng.uniform(0.5, 9.5, gt.shape)
    return pred, gt


def test_gradient_matches_central_differences():
    pred, gt = _small()
    h = 1e-6
    for per_image in (False, True):
        loss, grad, tie = grad_match_ref(pred, gt, scales=4, per_image=per_image)
        assert loss > 0 and not tie.any()
        num = np.zeros_like(pred)
        for idx in np.ndindex(*pred.shape):
            up, dn = pred.copy(), pred.copy()
            up[idx] += h
            dn[idx] -= h
            num[idx] = (grad_match_ref(up, gt, scales=4, per_image=per_image)[0]
                        - grad_match_ref(dn, gt, scales=4, per_image=per_image)[0]) / (2 * h)
        # |dR| is far from 0 on this data (no tie), so the loss is smooth within +-h: the
        # truncation error is ~h^2 f''' ~ 1e-11, the rounding error ~ eps * loss / h ~ 1e-9
        np.testing.assert_allclose(grad, num, rtol=0, atol=1e-7)
        assert (grad[gt <= 1e-3] == 0).all() and np.abs(grad).max() > 1e-3


def test_invariant_to_the_scale_of_the_prediction():
    pred, gt = _small(seed=4)
    for per_image in (False, True):
        l1, g1, _ = grad_match_ref(pred, gt, per_image=per_image)
        l3, g3, _ = grad_match_ref(3.0 * pred, gt, per_image=per_image)
        assert abs(l3 - l1) <= 1e-7
        np.testing.assert_allclose(3.0 * g3, g1, rtol=0, atol=1e-7)


def test_hand_computed_2x3():
    # R = [[0, 1, 3], [2, 2, invalid]]
    R = np.array([[[0.0, 1.0, 3.0], [2.0, 2.0, 0.0]]])
    gt = np.array([[[1.0, 1.0, 1.0], [1.0, 1.0, 0.0]]])
    pred = np.exp(R)
    S, N = grad_match_sums(pred, gt, scales=2)
    # scale 0: rows |1-0| + |3-1| + |2-2|, columns |2-0| + |2-1|; 5 valid pixels
    # scale 1: grid pixels (0,0) and (0,2): |3-0|; 2 valid grid pixels
    np.testing.assert_allclose(S, [[6.0, 3.0]], atol=1e-12)
    np.testing.assert_array_equal(N, [[5.0, 2.0]])
    for per_image in (False, True):  # one image: the two normalisers agree
        loss, grad, tie = grad_match_ref(pred, gt, scales=2, per_image=per_image)
        assert abs(loss - (6 / 5 + 3 / 2)) <= 1e-12 and not tie.any()
        # c_0 = [[-2, -1, +1], [+1 (sign(0) = 0 on its right pair), +1, -]], c_1 = -1 at (0,0), +1 at (0,2)
        dR = np.array([[[-2 / 5 - 1 / 2, -1 / 5, 1 / 5 + 1 / 2], [1 / 5, 1 / 5, 0.0]]])
        np.testing.assert_allclose(grad, dR / pred, rtol=0, atol=1e-12)
        assert grad[0, 1, 2] == 0.0
    # one scale only
    assert abs(grad_match_ref(pred, gt, scales=1)[0] - 6 / 5) <= 1e-12


def test_per_image_and_per_batch_normalisers():
    pred, gt = _small(seed=5, B=3)
    gt[1, :, 4:] = 0.0  # image 1 has fewer valid pixels than image 0
    gt[2] = 0.0  # image 2 has none: it leaves the per-image mean and adds nothing per batch
    S, N = grad_match_sums(pred, gt, scales=3)
    assert N[0, 0] > N[1, 0] > 0 and (N[2] == 0).all() and (S[2] == 0).all()
    lb, gb, _ = grad_match_ref(pred, gt, scales=3, per_image=False)
    li, gi, _ = grad_match_ref(pred, gt, scales=3, per_image=True)
    assert abs(lb - sum((S[0, k] + S[1, k]) / (N[0, k] + N[1, k]) for k in range(3))) <= 1e-12
    assert abs(li - 0.5 * sum(S[0, k] / N[0, k] + S[1, k] / N[1, k] for k in range(3))) <= 1e-12
    assert abs(li - lb) > 1e-3
    singles = [grad_match_ref(pred[b:b + 1], gt[b:b + 1], scales=3, per_image=True) for b in range(3)]
    assert singles[2][0] == 0.0 and not singles[2][1].any()
    assert abs(li - 0.5 * (singles[0][0] + singles[1][0])) <= 1e-12
    np.testing.assert_allclose(gi[:2], 0.5 * np.concatenate([singles[0][1], singles[1][1]]), rtol=0, atol=1e-12)
    assert not gi[2].any() and not gb[2].any()
    # no valid pixel anywhere: 0, gradient 0, nothing non-finite
    for per_image in (False, True):
        l0, g0, _ = grad_match_ref(pred, np.zeros_like(gt), per_image=per_image)
        assert l0 == 0.0 and not g0.any()


def test_shared_gpu_inputs_keep_the_near_tie_exclusion_small():
    """The GPU tests exclude near-tie pixels from the gradient check; on their inputs that is at
    most 1 % of the valid pixels (they assert the same cap)."""
    for B, H, W, keep in SHAPES:
        pred, gt = make_inputs(B, H, W, keep)
        assert pred.dtype == np.float32 and (gt[:, :3] == 0).all() and (pred > 0).all()
        valid = gt > 1e-3
        assert abs(valid[:, 3:].mean() - keep) < 0.05
        _, _, tie = grad_match_ref(pred, gt, scales=4)
        assert tie.sum() <= 0.01 * valid.sum()
