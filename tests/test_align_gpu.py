"""Scale- and shift-aligned depth metrics (cfg eval.align; csrc/align.hip, mf.depth_align and
mf.depth_metrics(align=...)) against the fp64 reference of tests/align_ref.py."""
import numpy as np
import pytest
import torch

import align_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [pytest.param(shape, mode, id=f"{shape[1]}x{shape[2]}-{mode}") for shape in A.SHAPES for mode in A.MODES]
# the evaluator's own rectangle: KITTI's eigen crop (under the garg crop one pixel of the sparse
# shape sits 4e-6 from a delta cut in lstsq_disp, which check_preconditions refuses)
CROP = {"garg_crop": False, "eigen_crop": True, "min_depth_eval": A.DMIN, "max_depth_eval": A.DMAX}


@pytest.fixture(scope="module")
def mf():
    from mdemi import _lib
    from mdemi import functional as mf
    _lib.load()
    A.check_preconditions()
    return mf


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared inputs are read-only


def bits(t):
    """The bit pattern of a tensor, so that equal means bit-equal (NaN included)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def run(mf, pred, gt, mode, rect=None, **kw):
    rect = A.rect_of(*pred.shape[-2:]) if rect is None else rect
    return mf.depth_metrics(pred, gt, rect, A.DMIN, A.DMAX, align=mode, **kw)


def check_coef(coef, ref, gt, mask, mode):
    """Test 1's bounds.  median: s within 4 fp64 ulp, t exactly 0.  Least squares: 1e-9 relative --
    fp64 sums of n <= 1e4 terms in another order differ by <= n 2^-53 ~ 1e-12 relative, the det
    cancellation amplifies that by ~1/cv^2 <= 12, which leaves ~100x margin; an fp32 accumulation
    is off by 4e-8 or more."""
    assert coef.shape == ref.shape
    assert np.array_equal(coef[:, 2], ref[:, 2]), ("n", coef[:, 2], ref[:, 2])
    assert np.array_equal(coef[:, 3], ref[:, 3]), ("status", coef[:, 3], ref[:, 3])
    for b in range(coef.shape[0]):
        s, t, s_ref, t_ref = coef[b, 0], coef[b, 1], ref[b, 0], ref[b, 1]
        if mode == "median":
            print(f"image {b}: s {s!r} ref {s_ref!r} ulp {int(A.ulp_diff64(s, s_ref))}")
            assert A.ulp_diff64(s, s_ref) <= 4, (b, s, s_ref)
            assert t == 0.0
        else:
            y = gt[b][mask[b]].astype(np.float64)  # the shift is measured against the size of the target
            y = 1.0 / y if mode == "lstsq_disp" else y
            t_scale = abs(t_ref) + np.abs(y).mean()
            print(f"image {b}: ds {abs(s - s_ref) / abs(s_ref):.3e} dt {abs(t - t_ref) / t_scale:.3e}")
            assert abs(s - s_ref) <= 1e-9 * abs(s_ref), (b, s, s_ref)
            assert abs(t - t_ref) <= 1e-9 * t_scale, (b, t, t_ref)


@pytest.mark.parametrize("shape,mode", CASES)
def test_coef_matches_reference(mf, shape, mode):
    pred, gt = A.make_inputs(*shape)
    ref = A.reference(*shape, mode)
    coef = mf.depth_align(dev(pred)[:, None], dev(gt)[:, None], A.rect_of(*shape[1:3]), A.DMIN, A.DMAX, mode)
    assert coef.shape == (shape[0], 4) and coef.dtype == torch.float64
    check_coef(coef.cpu().numpy(), ref["coef"], gt, ref["mask"], mode)


@pytest.mark.parametrize("kind", ["five_values", "low_mantissa_bits"])
def test_median_corner_cases(mf, kind):
    """Heavy ties (the rank lands inside a run of equal keys in every pass) and predictions that
    differ only in their lowest 8 mantissa bits (the first two passes see one bin, the last one
    decides); the batch's n are 747, 750 and 765, so odd and even."""
    shape = A.SHAPES[0]
    _, gt = A.make_inputs(*shape)
    rng = np.random.default_rng(3)
    if kind == "five_values":
        pred = np.float32([1.5, 2.5, 4.0, 7.0, 12.0])[rng.integers(0, 5, gt.shape)]
    else:
        pred = (np.uint32(0x40000000) | rng.integers(0, 256, gt.shape).astype(np.uint32)).view(np.float32)
    rect = A.rect_of(*shape[1:3])
    ref = A.align_ref(pred, gt, rect, "median")
    assert {int(n) % 2 for n in ref["coef"][:, 2]} == {0, 1}
    coef = mf.depth_align(dev(pred)[:, None], dev(gt)[:, None], rect, A.DMIN, A.DMAX, "median").cpu().numpy()
    check_coef(coef, ref["coef"], gt, ref["mask"], "median")


@pytest.mark.parametrize("shape,mode", CASES)
def test_aligned_map_and_fusion(mf, shape, mode):
    """The aligned map is within 1 fp32 ulp of the reference q on every pixel, off the valid set
    too (1 ulp: the build contracts s p + t into an fma); the fused metrics are, bit for bit,
    the unaligned kernel's on that map; and they match the fp64 reference pipeline."""
    pred, gt = A.make_inputs(*shape)
    ref = A.reference(*shape, mode)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    out, aligned = run(mf, p, g, mode, return_aligned=True)
    assert out.shape == (shape[0], 12) and out.dtype == torch.float64 and aligned.shape == p.shape
    ulp = A.ulp_diff32(aligned.cpu().numpy()[:, 0], ref["q"])
    print("aligned map: max ulp", int(ulp.max()), "pixels off by one", int((ulp == 1).sum()))
    assert ulp.max() <= 1
    plain = mf.depth_metrics(aligned, g, A.rect_of(*shape[1:3]), A.DMIN, A.DMAX)
    assert torch.equal(bits(out[:, :10]), bits(plain))
    assert torch.equal(bits(out), bits(run(mf, p, g, mode)))  # with and without the map
    coef = mf.depth_align(p, g, A.rect_of(*shape[1:3]), A.DMIN, A.DMAX, mode)
    assert torch.equal(bits(out[:, 10:]), bits(coef[:, :2]))
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 9], ref["coef"][:, 2])
    for b in range(shape[0]):
        for i, name in enumerate(A.METRICS):
            r = ref["metrics"][b, i]
            assert abs(got[b, i] - r) <= 2e-6 * abs(r) + 1e-9, (b, name, got[b, i], r)


@pytest.mark.parametrize("shape,mode", CASES)
def test_tcompute_errors_gpu_with_eval_align(mf, shape, mode):
    """End to end: eval.align through tcompute_errors_gpu (its own crop rectangle) against the
    fp64 reference pipeline, at the existing metric test's bound."""
    from mdemi.utils.depth_utils import METRICS, eval_crop_rect, tcompute_errors_gpu
    pred, gt = A.make_inputs(*shape)
    rect = eval_crop_rect(CROP, shape[1], shape[2], "KITTI")
    A.check_preconditions([shape], rect)
    ref = A.reference(*shape, mode, rect)
    rows = tcompute_errors_gpu(dev(pred)[:, None], dev(gt)[:, None], {**CROP, "align": mode}, "KITTI")
    assert len(rows) == shape[0]
    for b, row in enumerate(rows):
        assert tuple(row) == METRICS == A.METRICS
        for i, name in enumerate(METRICS):
            r = ref["metrics"][b, i]
            print(f"image {b} {name}: {row[name]!r} ref {r!r}")
            assert abs(row[name] - r) <= 2e-6 * abs(r) + 1e-9, (b, name, row[name], r)


@pytest.mark.parametrize("mode", A.MODES)
def test_failure_rule(mf, mode):
    """No valid pixel; a constant prediction (det = 0: with p = 2 every sum is exact in any order,
    so det is exactly 0; the median mode aligns it); a negative constant (median(p) <= 0, det = 0);
    NaN predictions (a NaN det; any s under median, but no fault or hang).  A failed image has
    status 1, s = 1, t = 0 and the unaligned call's metrics, bit for bit."""
    shape = A.SHAPES[0]
    base_pred, base_gt = A.make_inputs(*shape)
    H, W = shape[1:3]
    rng = np.random.default_rng(5)
    gt = np.stack([np.zeros((H, W), np.float32), base_gt[0], base_gt[1], base_gt[2]])
    pred = np.stack([base_pred[0], np.full((H, W), 2.0, np.float32), np.full((H, W), -1.0, np.float32),
                     np.where(rng.uniform(size=(H, W)) < 0.1, np.float32(np.nan), base_pred[2])])
    rect = A.rect_of(H, W)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    out, aligned = run(mf, p, g, mode, return_aligned=True)
    coef = mf.depth_align(p, g, rect, A.DMIN, A.DMAX, mode).cpu().numpy()
    plain = mf.depth_metrics(p, g, rect, A.DMIN, A.DMAX)
    n = A.valid_mask(gt, rect).reshape(4, -1).sum(1)
    assert np.array_equal(coef[:, 2], n) and n[0] == 0
    failed = [0, 2] if mode == "median" else [0, 1, 2, 3]
    for b in failed:
        assert coef[b].tolist() == [1.0, 0.0, float(n[b]), 1.0], (b, coef[b])
        assert torch.equal(bits(out[b, :10]), bits(plain[b])), b
        assert out[b, 10:].tolist() == [1.0, 0.0]
        assert torch.equal(bits(aligned[b]), bits(p[b])), b
    if mode == "median":
        ref = A.align_ref(pred[1:2], gt[1:2], rect, "median")["coef"][0]
        assert coef[1, 3] == 0.0 and A.ulp_diff64(coef[1, 0], ref[0]) <= 4 and coef[1, 1] == 0.0
        assert coef[3, 3] in (0.0, 1.0)


@pytest.mark.parametrize("mode", A.MODES)
def test_deterministic_and_layout_independent(mf, mode):
    """Two runs give the same bits; so do a non-contiguous pred and bases offset by one float
    (4-byte aligned only) against a contiguous copy."""
    shape = A.SHAPES[1]
    pred, gt = A.make_inputs(*shape)
    B, H, W = shape[:3]
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    rect = A.rect_of(H, W)

    def all_bits(p, g):
        out, aligned = run(mf, p, g, mode, return_aligned=True)
        coef = mf.depth_align(p, g, rect, A.DMIN, A.DMAX, mode)
        return bits(out), bits(aligned), bits(coef)

    want = all_bits(p, g)
    assert all(torch.equal(a, b) for a, b in zip(want, all_bits(p, g)))
    wide = torch.zeros(B, 1, H, W + 3, device=DEV)
    wide[..., 1:W + 1] = p
    strided = wide[..., 1:W + 1]
    assert not strided.is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(want, all_bits(strided, g)))
    flat_p, flat_g = torch.zeros(p.numel() + 1, device=DEV), torch.zeros(g.numel() + 1, device=DEV)
    flat_p[1:] = p.reshape(-1)
    flat_g[1:] = g.reshape(-1)
    off_p, off_g = flat_p[1:].view(p.shape), flat_g[1:].view(g.shape)
    assert off_p.data_ptr() % 16 == 4 and off_p.is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(want, all_bits(off_p, off_g)))


def test_median_workspace_aligned_to_8_bytes_only(mf):
    """mdemi_depth_align asks for an 8-byte-aligned workspace and no more: a workspace at 8 mod 16
    (the select's tables then sit at 8 mod 16 too) gives the bits of mf.depth_align's."""
    from mdemi import _lib as L
    lib = L.load()
    shape = A.SHAPES[1]
    pred, gt = A.make_inputs(*shape)
    B, H, W = shape[:3]
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    rect = A.rect_of(H, W)
    want = mf.depth_align(p, g, rect, A.DMIN, A.DMAX, "median")
    ws = torch.zeros(lib.mdemi_depth_align_workspace_size(B, H, W, L.ALIGN_MEDIAN) + 16, device=DEV, dtype=torch.uint8)
    assert ws.data_ptr() % 16 == 0
    coef = torch.empty(B, 4, device=DEV, dtype=torch.float64)
    L.check(lib.mdemi_depth_align(p.data_ptr(), g.data_ptr(), B, H, W, *rect, A.DMIN, A.DMAX, L.ALIGN_MEDIAN,
                                  coef.data_ptr(), ws.data_ptr() + 8, L.stream()), "depth_align")
    assert torch.equal(bits(coef), bits(want))


def test_default_is_untouched(mf):
    """Without align, depth_metrics returns its ten columns and tcompute_errors_gpu its nine keys,
    with the values of the unaligned prediction; "none" is the same as no key."""
    from mdemi.utils.depth_utils import METRICS, eval_crop_rect, tcompute_errors_gpu
    shape = A.SHAPES[0]
    pred, gt = A.make_inputs(*shape)
    p, g = dev(pred)[:, None], dev(gt)[:, None]
    rect = A.rect_of(*shape[1:3])
    out = mf.depth_metrics(p, g, rect, A.DMIN, A.DMAX)
    assert out.shape == (shape[0], 10) and out.dtype == torch.float64
    mask = A.valid_mask(gt, rect)
    got = out.cpu().numpy()
    for b in range(shape[0]):
        ref = A.metrics_of(gt[b][mask[b]], np.clip(pred[b][mask[b]], np.float32(A.DMIN), np.float32(A.DMAX)))
        assert got[b, 9] == mask[b].sum()
        for i in range(9):
            assert abs(got[b, i] - ref[i]) <= 2e-6 * abs(ref[i]) + 1e-9, (b, i, got[b, i], ref[i])
    rows = tcompute_errors_gpu(p, g, CROP, "KITTI")
    plain = mf.depth_metrics(p, g, eval_crop_rect(CROP, shape[1], shape[2], "KITTI"), A.DMIN, A.DMAX).cpu().numpy()
    assert [tuple(r) for r in rows] == [METRICS] * shape[0]
    assert rows == [dict(zip(METRICS, r[:9].tolist())) for r in plain]
    assert rows == tcompute_errors_gpu(p, g, {**CROP, "align": "none"}, "KITTI")
    with pytest.raises(ValueError, match="eval.align"):
        tcompute_errors_gpu(p, g, {**CROP, "align": "mean"}, "KITTI")
    with pytest.raises(ValueError, match="align"):
        mf.depth_metrics(p, g, rect, A.DMIN, A.DMAX, align="none")


def test_abi_refuses_bad_arguments(mf):
    from mdemi import _lib as L
    lib = L.load()
    x = torch.ones(64, device=DEV)
    c = torch.zeros(4, device=DEV, dtype=torch.float64)
    ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    args = (x.data_ptr(), x.data_ptr(), 1, 8, 8, 0, 8, 0, 8, 1e-3, 80.0)
    assert lib.mdemi_depth_align_workspace_size(2, 37, 53, L.ALIGN_MEDIAN) >= 2 * 4 * 2048 * 4
    assert lib.mdemi_depth_align_workspace_size(2, 70, 131, L.ALIGN_LSTSQ) >= 2 * 3 * 5 * 8
    assert lib.mdemi_depth_align(*args, 0, c.data_ptr(), ws.data_ptr(), L.stream()) < 0
    assert b"mode" in lib.mdemi_last_error()
    assert lib.mdemi_depth_align(*args, 4, c.data_ptr(), ws.data_ptr(), L.stream()) < 0
    assert lib.mdemi_depth_align(*args, L.ALIGN_LSTSQ, c.data_ptr(), None, L.stream()) < 0
    assert lib.mdemi_depth_align(*args, L.ALIGN_LSTSQ, None, ws.data_ptr(), L.stream()) < 0
    assert lib.mdemi_depth_metrics_aligned(*args, 1, 0, c.data_ptr(), None, c.data_ptr(), ws.data_ptr(),
                                           L.stream()) < 0
    assert lib.mdemi_depth_metrics_aligned(*args, 1, L.ALIGN_MEDIAN, None, None, c.data_ptr(), ws.data_ptr(),
                                           L.stream()) < 0
