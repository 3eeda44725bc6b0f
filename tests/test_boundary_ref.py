"""eval.boundary on the CPU: depth_utils.boundary_counts / boundary_f1 (the numpy counterpart of
mdemi_depth_boundary) against the plain-slicing reference of tests/boundary_ref.py, the prefix
property the kernel's level histograms rest on, a hand-made map and the no-score rule."""
import numpy as np
import pytest

import boundary_ref as R


def test_reference_preconditions_hold():
    R.check_preconditions()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[1]}x{s[2]}")
@pytest.mark.parametrize("clamp", [True, False])
def test_counterpart_equals_the_reference(shape, clamp):
    """Counts exactly, scores to 1e-12."""
    from mdemi.utils.depth_utils import BOUNDARY_KEYS, boundary_counts, boundary_f1, boundary_thresholds
    assert BOUNDARY_KEYS == ("boundary_f1", "boundary_precision", "boundary_recall")
    thr = boundary_thresholds(R.T_MIN, R.T_MAX, R.N_T)
    assert thr.dtype == np.float32 and np.array_equal(thr, R.thresholds())
    assert np.array_equal(boundary_thresholds(), thr)  # the defaults
    pred, gt = R.make_inputs(*shape)
    ref = R.reference(*shape, clamp)
    q = R.evaluated(pred, clamp)
    for b in range(shape[0]):
        counts = boundary_counts(gt[b], q[b], ref["mask"][b], thr)
        assert counts.dtype == np.int64 and np.array_equal(counts, ref["counts"][b])
        got = boundary_f1(counts, thr)
        assert tuple(got) == BOUNDARY_KEYS
        for k, want in zip(BOUNDARY_KEYS, ref["out"][b, :3]):
            assert abs(got[k] - want) <= 1e-12 * abs(want), (b, k, got[k], want)


def test_thresholds_are_validated():
    from mdemi.utils.depth_utils import boundary_counts, boundary_f1, boundary_thresholds
    assert boundary_thresholds(1.1, 1.1, 1).tolist() == [np.float32(1.1)]
    assert boundary_thresholds(1.05, 2.0, 16).size == 16
    for bad, key in (((1.0, 1.25, 10), "t_min"), ((1.3, 1.25, 10), "t_max"), ((1.05, 1.25, 0), "n"),
                     ((1.05, 1.25, 17), "n"), ((1.05, 1.25, 2.0), "n"), ((True, 1.25, 10), "t_min"),
                     ((1.05, float("inf"), 10), "t_max")):
        with pytest.raises(ValueError, match=key):
            boundary_thresholds(*bad)
    with pytest.raises(ValueError, match="rounds to 1"):
        boundary_thresholds(1.0 + 1e-9, 1.25, 10)
    m = np.ones((3, 4), np.float32)
    for bad in (np.float64([1.1]), np.float32([1.0, 1.1]), np.float32([1.2, 1.1]), np.float32([]),
                np.full(17, 1.1, np.float32)):
        with pytest.raises(ValueError, match="thresholds"):
            boundary_counts(m, m, m > 0, bad)
    with pytest.raises(ValueError, match="counts"):
        boundary_f1(np.zeros((2, 4, 3), np.int64), np.float32([1.1]))


def test_passed_thresholds_form_a_prefix():
    """fl32(tau x) is monotone in tau for x >= 0: on 2e5 random pairs, a pair that passes tau_i
    passes every lower threshold, and the two kinds of a direction exclude each other."""
    rng = np.random.default_rng(7)
    n = 200_000
    a = np.exp(rng.uniform(np.log(1e-3), np.log(80.0), n)).astype(np.float32)
    ratio = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0.7, 1.4, n), np.exp(rng.uniform(-2, 2, n)))
    b = (a * ratio).astype(np.float32)
    a[:100], b[100:200] = 0.0, 0.0  # zeros pass every threshold or none
    thr = R.thresholds()
    far_b = np.stack([b > t * a for t in thr])  # (n_t, n)
    far_a = np.stack([a > t * b for t in thr])
    assert far_b.any() and far_a.any() and not far_b.all() and not far_a.all()
    for e in (far_b, far_a):
        level = e.sum(0)
        assert np.array_equal(e, np.arange(len(thr))[:, None] < level[None, :])
        assert len(np.unique(level)) == len(thr) + 1  # every level occurs
    assert not (far_b[0] & far_a[0]).any()
    # with a negative value neither holds: the thresholds passed are a suffix, and both kinds can pass
    assert (np.float32(-1.2) > thr * np.float32(-1.0)).tolist() == [False] * 7 + [True] * 3
    assert np.float32(-1.0) > thr[0] * np.float32(-1.2)


def test_hand_made_map():
    """3 x 4, thresholds 1.1 and 2.0; the pixel at (2, 3) is invalid.
         g = 1 1 2 2      q = 1 2 2 2
             1 1 2 2          1 1 1 3
             4 4 4 .          4 4 4 .
    """
    from mdemi.utils.depth_utils import boundary_counts, boundary_f1
    g = np.float32([[1, 1, 2, 2], [1, 1, 2, 2], [4, 4, 4, 9]])
    q = np.float32([[1, 2, 2, 2], [1, 1, 1, 3], [4, 4, 4, 9]])
    valid = np.ones((3, 4), bool)
    valid[2, 3] = False
    thr = np.float32([1.1, 2.0])
    c = boundary_counts(g, q, valid, thr)
    # horizontal pairs: rows 0 and 1 have 3 each, row 2 has 2; vertical: 3 columns of 2, column 3 of 1
    # tau = 1.1, kind 0 (right is farther): g at (0,1)-(0,2), (1,1)-(1,2); q at (0,0)-(0,1), (1,2)-(1,3)
    assert c[0, 0].tolist() == [2, 2, 0]
    assert c[0, 1].tolist() == [0, 0, 0]
    # kind 2 (lower is farther): g rows 1 -> 2 in columns 0..2; q the same three, and (0,3)-(1,3): 2 -> 3
    assert c[0, 2].tolist() == [3, 4, 3]
    # kind 3 (upper is farther): q at (0,1)-(1,1): 2 over 1, and (0,2)-(1,2)
    assert c[0, 3].tolist() == [0, 2, 0]
    # tau = 2: strict, so 1 -> 2 is no edge (2 > 2.0 * 1 fails); 1 -> 4 and 1 -> 3 are
    assert c[1, 0].tolist() == [0, 1, 0]   # q (1,2)-(1,3): 3 > 2
    assert c[1, 1].tolist() == [0, 0, 0]
    assert c[1, 2].tolist() == [2, 3, 2]   # g: columns 0, 1 (1 -> 4); q: columns 0, 1, 2
    assert c[1, 3].tolist() == [0, 0, 0]
    assert np.array_equal(c, R.counts_of(g, q, valid, thr)[0])
    s = boundary_f1(c, thr)
    p0, r0 = 0.25 * (0 / 2 + 0 + 3 / 4 + 0 / 2), 0.25 * (0 / 2 + 0 + 3 / 3 + 0)
    p1, r1 = 0.25 * (0 / 1 + 0 + 2 / 3 + 0), 0.25 * (0 + 0 + 2 / 2 + 0)
    t = thr.astype(np.float64)
    w = t / t.sum()
    f = [2 * p * r / (p + r) for p, r in ((p0, r0), (p1, r1))]
    assert abs(s["boundary_precision"] - (w[0] * p0 + w[1] * p1)) < 1e-15
    assert abs(s["boundary_recall"] - (w[0] * r0 + w[1] * r1)) < 1e-15
    assert abs(s["boundary_f1"] - (w[0] * f[0] + w[1] * f[1])) < 1e-15
    # invariance to a depth scale, and a perfect prediction
    assert np.array_equal(boundary_counts(g, 2 * q, valid, thr)[..., 1:], c[..., 1:])
    perfect = boundary_f1(boundary_counts(g, g, valid, thr), thr)
    # a kind without an edge counts 0 in the mean over the four: two kinds have edges at 1.1, one at 2
    assert abs(perfect["boundary_f1"] - (w[0] * 0.5 + w[1] * 0.25)) < 1e-15
    assert perfect["boundary_precision"] == perfect["boundary_recall"]


def test_no_edge_ground_truth_has_no_score():
    from mdemi.utils.depth_utils import boundary_counts, boundary_f1
    thr = R.thresholds()
    flat = np.full((6, 7), 3.0, np.float32)
    q = flat * np.float32(1.0) + np.arange(7, dtype=np.float32)
    c = boundary_counts(flat, q, np.ones((6, 7), bool), thr)
    assert c[..., 0].sum() == 0 and c[..., 1].sum() > 0 and c[..., 2].sum() == 0
    assert boundary_f1(c, thr) is None
    assert R.scores_of(c, thr) == (0.0, 0.0, 0.0, 1)
    # sparse returns with no two adjacent: no pair at all
    sparse = np.zeros((6, 8), bool)
    sparse[::2, ::2] = True
    g = np.where(sparse, np.float32(2.0), np.float32(0.0)) * np.linspace(1, 3, 8, dtype=np.float32)
    c = boundary_counts(g, g, sparse, thr)
    assert c.sum() == 0 and boundary_f1(c, thr) is None
    assert R.counts_of(g, g, sparse, thr)[1] == 0
