"""Scale-invariant boundary F1 on the GPU (cfg eval.boundary; csrc/boundary.hip, mf.depth_boundary)
against the plain-numpy reference of tests/boundary_ref.py: integer counts exactly, fp64 scores to
1e-12 relative."""
import ctypes

import numpy as np
import pytest
import torch

import boundary_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [pytest.param(shape, id=f"{shape[1]}x{shape[2]}") for shape in R.SHAPES]
CROP = {"garg_crop": False, "eigen_crop": True, "min_depth_eval": R.DMIN, "max_depth_eval": R.DMAX}


@pytest.fixture(scope="module")
def mf():
    from mdemi import _lib
    from mdemi import functional as mf
    _lib.load()
    R.check_preconditions()
    return mf


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared inputs are read-only


def bits(t):
    """The bit pattern of a tensor, so that equal means bit-equal."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def run(mf, pred, gt, rect=None, thr=None, **kw):
    rect = R.rect_of(*pred.shape[-2:]) if rect is None else rect
    return mf.depth_boundary(pred, gt, rect, R.DMIN, R.DMAX, thresholds=R.thresholds() if thr is None else thr,
                             return_counts=True, **kw)


def check(out, counts, ref):
    """Counts, n_pairs and status exactly; the three scores within 1e-12 relative of the fp64
    reference (a few dozen fp64 operations on exact integer counts: each rounds by 2^-53)."""
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert counts.dtype == np.int64 and counts.shape == ref["counts"].shape
    assert np.array_equal(counts, ref["counts"]), np.argwhere(counts != ref["counts"])[:8]
    assert out.shape == ref["out"].shape and out.dtype == np.float64
    assert np.array_equal(out[:, 3:], ref["out"][:, 3:]), (out[:, 3:], ref["out"][:, 3:])
    for b in range(out.shape[0]):
        for j in range(3):
            print(f"image {b} score {j}: {out[b, j]!r} ref {ref['out'][b, j]!r}")
            assert abs(out[b, j] - ref["out"][b, j]) <= 1e-12 * abs(ref["out"][b, j]), (b, j)


@pytest.mark.parametrize("shape", CASES)
def test_counts_and_scores_match_the_reference(mf, shape):
    pred, gt = R.make_inputs(*shape)
    B, H, W = shape[:3]
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    out, counts = run(mf, p, g)
    assert out.shape == (B, 5) and out.dtype == torch.float64 and counts.shape == (B, R.N_T, 4, 3)
    check(out, counts, R.reference(*shape))
    assert torch.equal(bits(out), bits(mf.depth_boundary(p, g, R.rect_of(H, W), R.DMIN, R.DMAX)))  # default thresholds
    # the whole image as the rectangle: the sweep's own edges are the image's
    full = (0, H, 0, W)
    check(*run(mf, p, g, rect=full), R.reference(*shape, True, full))


def test_the_large_shape_spans_row_chunks(mf):
    from mdemi import _lib as L
    lib = L.load()
    B, H, W, _ = R.SHAPES[4]
    assert lib.mdemi_depth_boundary_row_chunks(H, W) >= 3
    assert lib.mdemi_depth_boundary_row_chunks(*R.SHAPES[0][1:3]) == 1
    assert W % 4 == 0 and R.SHAPES[1][2] % 4 == 0 and R.SHAPES[0][2] % 4 != 0  # both load paths are run


def test_both_load_paths_agree(mf):
    """Bases offset by one float (4-byte aligned only) take the scalar path on a W % 4 == 0 shape:
    the same counts, the same bits as the vector path's."""
    shape = R.SHAPES[4]
    pred, gt = R.make_inputs(*shape)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    want = run(mf, p, g)
    flat_p, flat_g = torch.zeros(p.numel() + 1, device=DEV), torch.zeros(g.numel() + 1, device=DEV)
    flat_p[1:] = p.reshape(-1)
    flat_g[1:] = g.reshape(-1)
    off_p, off_g = flat_p[1:].view(p.shape), flat_g[1:].view(g.shape)
    assert off_p.data_ptr() % 16 == 4 and off_p.is_contiguous()
    got = run(mf, off_p, off_g)
    assert torch.equal(want[1], got[1]) and torch.equal(bits(want[0]), bits(got[0]))


@pytest.mark.parametrize("width", [64, 63])
def test_ties(mf, width):
    """Pairs (1, tau_i) and (1, nextafter(tau_i, 2)) for every i, in both orders and both
    directions: the first is no edge at tau_i (strict compare, fl32(tau_i * 1) = tau_i), the second
    is one.  A >=, a division or a contracted multiply-compare would move one of them."""
    thr = R.thresholds()
    up = np.nextafter(thr, np.float32(2))
    g = np.ones((2, 2 * len(thr) + 2, width), np.float32)
    for i in range(len(thr)):  # image 0: horizontal pairs at columns (4 k, 4 k + 1); image 1: vertical pairs
        g[0, 2 * i, 1::4], g[0, 2 * i + 1, 1::4] = thr[i], up[i]
        g[0, 2 * i, 2::4], g[0, 2 * i + 1, 2::4] = thr[i], up[i]  # (tau, tau) next to it: no edge; then tau -> 1
        g[1, 2 * i, i::len(thr) + 1] = thr[i] if i % 2 == 0 else up[i]
    q = np.ascontiguousarray(g[:, ::-1, ::-1])  # the prediction: the same pairs in the other order
    H, W = g.shape[1:]
    rect = (0, H, 0, W)
    ref = R.boundary_ref(q, g, rect, thr)
    c = ref["counts"]
    # image 0, kind 0 (right is farther), 1 -> t over the 16 columns 0, 4, ...: at tau_i the rows of
    # up[j], j >= i, and of thr[j], j > i
    n_col = len(range(1, width, 4))
    for i in range(len(thr)):
        assert c[0, i, 0, 0] == n_col * (2 * (len(thr) - i) - 1), (i, c[0, i, 0])
    assert c[0, :, 1, 0].min() > 0 and c[1, :, 2, 0].min() > 0 and c[1, :, 3, 0].min() > 0
    out, counts = run(mf, dev(q)[:, None], dev(g)[:, None], rect=rect, thr=thr, clamp_pred=False)
    check(out, counts, ref)
    # and as its own prediction: every edge is a true positive, the scores are not 0
    same = R.boundary_ref(g, g, rect, thr)
    assert np.array_equal(same["counts"][..., 2], same["counts"][..., 0]) and (same["out"][:, 0] > 0.4).all()
    check(*run(mf, dev(g)[:, None], dev(g)[:, None], rect=rect, thr=thr), same)


def test_scale_invariance_and_clamp(mf):
    shape = R.SHAPES[0]
    pred, gt = R.make_inputs(*shape)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    # unclamped: a power of two scales every product exactly, the counts are identical
    out1, c1 = run(mf, p, g, clamp_pred=False)
    check(out1, c1, R.reference(*shape, False))
    out2, c2 = run(mf, p * 2, g, clamp_pred=False)
    assert torch.equal(c1, c2) and torch.equal(bits(out1), bits(out2))
    # clamped, a prediction partly out of range on both sides: the counts of the clamped map
    wide = (pred * np.float32(2.5) - np.float32(6.5)).astype(np.float32)
    assert (wide > R.DMAX).mean() > 0.05 and (wide < R.DMIN).mean() > 0.05
    rect = R.rect_of(*shape[1:3])
    assert (wide[R.valid_mask(gt, rect)] < 0).sum() > 100
    ref = R.boundary_ref(R.evaluated(wide, True), gt, rect)
    assert not np.array_equal(ref["counts"], R.boundary_ref(wide, gt, rect)["counts"])
    check(*run(mf, dev(wide)[:, None], g), ref)
    # unclamped, negative values included: still the counts of the definition
    check(*run(mf, dev(wide)[:, None], g, clamp_pred=False), R.boundary_ref(wide, gt, rect))


@pytest.mark.parametrize("mode", ["median", "lstsq", "lstsq_disp"])
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1]], ids=["37x53", "48x64"])
def test_aligned_counts_are_those_of_the_aligned_map(mf, shape, mode):
    """With align the sweep forms q itself (aligned_value, from coef on the device): the counts
    equal, bit for bit, the unaligned call's on the map depth_metrics(return_aligned=True) returns."""
    pred, gt = R.make_inputs(*shape)
    p, g = dev(pred * np.float32(0.37) + np.float32(0.8))[:, None], dev(gt)[:, None]
    rect = R.rect_of(*shape[1:3])
    _, aligned = mf.depth_metrics(p, g, rect, R.DMIN, R.DMAX, align=mode, return_aligned=True)
    for clamp in (True, False):
        out, counts = run(mf, p, g, align=mode, clamp_pred=clamp)
        want_out, want_counts = run(mf, aligned, g, clamp_pred=clamp)
        assert torch.equal(counts, want_counts) and torch.equal(bits(out), bits(want_out))
        check(out, counts, R.boundary_ref(R.evaluated(aligned.cpu().numpy()[:, 0], clamp), gt, rect))
    plain = run(mf, p, g)[1]
    assert not torch.equal(plain, counts) or mode == "median"  # the alignment is not a no-op here
    coef = mf.depth_align(p, g, rect, R.DMIN, R.DMAX, mode)
    again = run(mf, p, g, align=mode, coef=coef, clamp_pred=False)
    assert torch.equal(again[1], counts) and torch.equal(bits(again[0]), bits(out))


def test_deterministic_and_leaves_the_metrics_alone(mf):
    """Two runs give equal bits; the nine metrics on the same tensors are bit-equal before and
    after a boundary call (the three calls share one workspace slot)."""
    shape = R.SHAPES[4]
    pred, gt = R.make_inputs(*shape)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    rect = R.rect_of(*shape[1:3])
    before = mf.depth_metrics(p, g, rect, R.DMIN, R.DMAX)
    before_al = mf.depth_metrics(p, g, rect, R.DMIN, R.DMAX, align="median")
    a = run(mf, p, g)
    b = run(mf, p, g)
    assert torch.equal(a[1], b[1]) and torch.equal(bits(a[0]), bits(b[0]))
    assert torch.equal(bits(before), bits(mf.depth_metrics(p, g, rect, R.DMIN, R.DMAX)))
    al = run(mf, p, g, align="median")
    assert torch.equal(bits(before_al), bits(mf.depth_metrics(p, g, rect, R.DMIN, R.DMAX, align="median")))
    assert torch.equal(al[1], run(mf, p, g, align="median")[1])


def test_graph_capture(mf):
    """The call neither synchronises nor allocates behind the stream: a captured call replays to
    the eager call's bits on new inputs."""
    shape = R.SHAPES[1]
    pred, gt = R.make_inputs(*shape)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    want = run(mf, p, g)
    sp, sg = torch.ones_like(p), torch.ones_like(g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(mf, sp, sg)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, counts = run(mf, sp, sg)
    sp.copy_(p)
    sg.copy_(g)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts, want[1]) and torch.equal(bits(out), bits(want[0]))


def test_flat_ground_truth_has_no_score(mf):
    """A flat ground truth has status 1 and scores 0; tcompute_errors_gpu then omits the three keys
    for that image only, and without eval.boundary it returns what it returned before."""
    from mdemi.utils.depth_utils import BOUNDARY_KEYS, METRICS, eval_crop_rect, tcompute_errors_gpu
    shape = R.SHAPES[1]
    pred, gt = R.make_inputs(*shape)
    gt = np.array(gt)
    gt[1] = 3.0
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    rect = eval_crop_rect(CROP, shape[1], shape[2], "KITTI")
    ref = R.boundary_ref(R.evaluated(pred), gt, rect)
    assert ref["out"][:, 4].tolist() == [0.0, 1.0] and ref["counts"][1, :, :, 1].sum() > 0
    out, counts = run(mf, p, g, rect=rect)
    check(out, counts, ref)
    assert out[1].tolist() == [0.0, 0.0, 0.0, ref["out"][1, 3], 1.0]
    plain = tcompute_errors_gpu(p, g, CROP, "KITTI")
    assert plain == tcompute_errors_gpu(p, g, {**CROP, "boundary": False}, "KITTI")
    assert [tuple(r) for r in plain] == [METRICS] * 2
    rows = tcompute_errors_gpu(p, g, {**CROP, "boundary": True}, "KITTI")
    assert tuple(rows[0]) == METRICS + BOUNDARY_KEYS and tuple(rows[1]) == METRICS
    assert [{k: r[k] for k in METRICS} for r in rows] == plain  # the same bits in the nine
    assert [rows[0][k] for k in BOUNDARY_KEYS] == out[0, :3].tolist()
    # other thresholds, and with an alignment: the scores of the aligned, clamped value
    ev = {**CROP, "boundary": {"t_min": 1.1, "t_max": 1.5, "n": 3}, "align": "lstsq"}
    rows = tcompute_errors_gpu(p, g, ev, "KITTI")
    thr = R.thresholds(1.1, 1.5, 3)
    m, aligned = mf.depth_metrics(p, g, rect, R.DMIN, R.DMAX, align="lstsq", return_aligned=True)
    want = R.boundary_ref(R.evaluated(aligned.cpu().numpy()[:, 0]), gt, rect, thr)
    assert tuple(rows[0]) == METRICS + BOUNDARY_KEYS and tuple(rows[1]) == METRICS
    for j, k in enumerate(BOUNDARY_KEYS):
        assert abs(rows[0][k] - want["out"][0, j]) <= 1e-12 * want["out"][0, j]
    assert [rows[b][k] for b in range(2) for k in METRICS] == m[:, :9].reshape(-1).tolist()
    with pytest.raises(ValueError, match=r"eval\.boundary\.n"):
        tcompute_errors_gpu(p, g, {**CROP, "boundary": {"n": 0}}, "KITTI")


def test_abi_refuses_bad_arguments(mf):
    """Host checks only: a negative code, a message, nothing launched."""
    from mdemi import _lib as L
    lib = L.load()
    x = torch.ones(64, device=DEV)
    c = torch.zeros(4, device=DEV, dtype=torch.float64)
    o = torch.full((5,), -7.0, device=DEV, dtype=torch.float64)
    ws = torch.zeros(1 << 12, device=DEV, dtype=torch.uint8)
    args = (x.data_ptr(), x.data_ptr(), 1, 8, 8, 0, 8, 0, 8, 1e-3, 10.0, 1)

    def thr(n, *t):
        s = L.BoundaryThresholds(n=n)
        s.t[:len(t)] = t
        return s

    def call(mode, coef, th, out=o.data_ptr(), w=ws.data_ptr(), a=args):
        return lib.mdemi_depth_boundary(*a, mode, coef, ctypes.addressof(th) if th is not None else None, None, out,
                                        w, L.stream())

    assert L.BOUNDARY_MAX_T == 16 and ctypes.sizeof(L.BoundaryThresholds) == 68
    assert lib.mdemi_depth_boundary_workspace_size(2, 10) >= 2 * 3 * 4 * 11 * 4
    assert lib.mdemi_depth_boundary_workspace_size(2, 0) == 0 == lib.mdemi_depth_boundary_workspace_size(2, 17)
    good = thr(2, 1.1, 1.2)
    assert call(0, None, thr(0)) < 0 and b"thresholds must be 1..16" in lib.mdemi_last_error()
    assert call(0, None, thr(17)) < 0 and b"thresholds must be 1..16" in lib.mdemi_last_error()
    assert call(L.ALIGN_LSTSQ, None, good) < 0 and b"coef" in lib.mdemi_last_error()
    assert call(0, c.data_ptr(), good) < 0 and b"coef" in lib.mdemi_last_error()
    assert call(4, c.data_ptr(), good) < 0 and b"mode" in lib.mdemi_last_error()
    assert call(0, None, thr(2, 1.0, 1.2)) < 0 and b"above 1" in lib.mdemi_last_error()
    assert call(0, None, thr(2, 1.2, 1.1)) < 0 and b"non-decreasing" in lib.mdemi_last_error()
    assert call(0, None, thr(1, float("inf"))) < 0
    assert call(0, None, None) < 0
    assert call(0, None, good, out=None) < 0
    assert call(0, None, good, w=None) < 0
    big = (x.data_ptr(), x.data_ptr(), 1, 1 << 15, 1 << 15, 0, 8, 0, 8, 1e-3, 10.0, 1)
    assert call(0, None, good, a=big) < 0 and b"2^30" in lib.mdemi_last_error()
    for B in (0, 65536):
        bad_b = (x.data_ptr(), x.data_ptr(), B, 8, 8, 0, 8, 0, 8, 1e-3, 10.0, 1)
        assert call(0, None, good, a=bad_b) < 0 and b"65535" in lib.mdemi_last_error()
    torch.cuda.synchronize()
    assert o.tolist() == [-7.0] * 5  # nothing ran
    assert call(0, None, good) == 0
    torch.cuda.synchronize()
    assert o.tolist() == [0.0, 0.0, 0.0, 2 * 8 * 7, 1.0]  # a flat 8 x 8 image: 112 pairs, no score
