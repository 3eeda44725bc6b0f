"""GPU checks of tiled inference's kernels (csrc/tile.hip through mdemi.functional): tile_extract
against torch slicing, tile_merge against the fp64 numpy reference of tests/tile_ref.py -- the
blend, the sequential per-tile alignment, the failure rule -- determinism, and the C ABI's
refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tile_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
B = 2
#        image      tile      overlap
CASES = [((37, 53), (16, 24), (5, 7)),    # 3 x 3, odd sizes: scalar paths, pixels under three tiles and more
         ((40, 56), (24, 32), (8, 8)),    # 2 x 2, vector paths
         ((20, 200), (32, 64), (0, 16)),  # 1 x 4, the tile clipped in y
         ((24, 32), (24, 32), (0, 0))]    # one tile
IDS = ["37x53", "40x56", "20x200", "24x32"]
MULTI = CASES[:3]
ALIGNS = ("lstsq", "lstsq_disp")
SEED, NOISE = 11, 1e-3


@pytest.fixture(scope="module")
def mf():
    import mdemi.functional as mf
    return mf


def _np(t):
    return t.cpu().numpy()


def _shifted(a):
    """a on the device as a contiguous view one float off the allocation's 16-byte alignment."""
    a = torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a
    buf = torch.zeros(a.numel() + 1, device=DEV, dtype=a.dtype)
    buf[1:] = a.reshape(-1).to(DEV)
    v = buf[1:].view(a.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@functools.lru_cache(maxsize=None)
def _case(size, tile, overlap, align):
    """(D, tiles fp32, reference (out, coef, blend), diag) -- computed once, never modified."""
    D, tiles = R.recoverable(size, tile, overlap, align, B=B, seed=SEED, noise=NOISE)
    diag = []
    ref = R.merge(tiles, size, tile, overlap, align, R.MAX_DEPTH, diag=diag)
    for a in (D, tiles, *ref):
        a.setflags(write=False)
    return D, tiles, ref, diag


def _plan(mf, size, tile, overlap):
    return mf.tile_plan(*size, tile, overlap)


@pytest.mark.parametrize("size,tile,overlap", CASES, ids=IDS)
def test_extract_is_torch_slicing(mf, size, tile, overlap):
    plan = _plan(mf, size, tile, overlap)
    rng = np.random.default_rng(2)
    img = torch.from_numpy(rng.standard_normal((B, 3) + size).astype(np.float32)).to(DEV)
    img[0, 0, 0, 0], img[1, 2, -1, -1] = float("nan"), float("-inf")
    th, tw = plan.tile
    want = torch.stack([img[b, :, y:y + th, x:x + tw] for b in range(B) for y in plan.ys for x in plan.xs])
    got = mf.tile_extract(img, plan)
    assert got.shape == want.shape == (B * len(plan.ys) * len(plan.xs), 3, th, tw)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    for other in (_shifted(img.cpu()), img.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):  # unaligned; strided
        assert torch.equal(mf.tile_extract(other, plan).view(torch.int32), got.view(torch.int32))
    with pytest.raises(ValueError, match="requires grad"):
        mf.tile_extract(img.clone().requires_grad_(), plan)
    with pytest.raises(ValueError, match="img must be"):
        mf.tile_extract(img[..., :-1], plan)


@pytest.mark.parametrize("size,tile,overlap", CASES, ids=IDS)
def test_blend_none_within_one_ulp(mf, size, tile, overlap):
    """The kernel and the reference do the same fp64 operations in the same order, except that the
    build contracts w * q + acc into an fma: the quotient can differ in its last fp64 bits and the
    one rounding to fp32 can then fall the other way -- 1 fp32 ulp at the most."""
    _, tiles, (want, _, _), _ = _case(size, tile, overlap, "none")
    plan = _plan(mf, size, tile, overlap)
    got, coef = mf.tile_merge(torch.from_numpy(tiles.copy()).to(DEV)[:, None], plan, size)
    assert coef is None and got.shape == (B, 1) + size and got.dtype == torch.float32
    d = R.ulp_diff(_np(got)[:, 0], want)
    print(f"blend none {size}: {int((d > 0).sum())} of {d.size} pixels off by one ulp, max {d.max():.2f}")
    assert d.max() <= 1
    again, _ = mf.tile_merge(_shifted(tiles), plan, size)  # (B*T,th,tw), unaligned: the scalar loads
    assert torch.equal(again, got)
    if tiles.shape[0] == B:  # one tile: its values, bit for bit
        assert np.array_equal(_np(got)[:, 0], tiles)
    with pytest.raises(ValueError, match="requires grad"):
        mf.tile_merge(torch.from_numpy(tiles.copy()).to(DEV).requires_grad_(), plan, size)
    with pytest.raises(ValueError, match="tile_pred must be"):
        mf.tile_merge(torch.from_numpy(tiles[:, :-1].copy()).to(DEV), plan, size)
    with pytest.raises(ValueError, match="plan is for"):
        mf.tile_merge(torch.from_numpy(tiles.copy()).to(DEV), plan, (size[0], size[1] + 1))


@pytest.mark.parametrize("size,tile", [((40, 56), (24, 32)), ((37, 53), (16, 24)), ((20, 200), (32, 64))],
                         ids=["40x56", "37x53", "20x200"])
def test_zero_overlap_keeps_the_tile_values(mf, size, tile):
    """Without an overlap every weight is 1: tiles cut from one map average back to it exactly
    ((q + q) / 2, 4 q / 4), NaN and inf included."""
    rng = np.random.default_rng(4)
    D = rng.uniform(0.5, 80.0, size=(B,) + size).astype(np.float32)
    D[0, 3, 5], D[1, -1, -1] = np.nan, np.inf
    tiles = R.cut(D, size, tile, (0, 0))
    got, _ = mf.tile_merge(torch.from_numpy(tiles).to(DEV), _plan(mf, size, tile, 0), size)
    assert np.array_equal(_np(got)[:, 0].view(np.int32), D.view(np.int32))


def test_fits_are_well_conditioned():
    """What the coefficient bound leans on, asserted on the CPU with the reference: no fit of the
    seeded inputs fails, each has hundreds of pairs, and x varies enough (cv >= 0.3) that the det
    cancellation amplifies a summation-order difference by no more than ~12."""
    for size, tile, overlap in MULTI:
        for align in ALIGNS:
            _, _, (_, coef, _), diag = _case(size, tile, overlap, align)
            assert not coef[..., 3].any() and coef[:, 1:, 2].min() >= 100
            assert len(diag) == B * (coef.shape[1] - 1)
            assert min(cv for _, _, cv, _ in diag) >= 0.3, (size, align, min(cv for _, _, cv, _ in diag))


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("size,tile,overlap", MULTI, ids=IDS[:3])
def test_aligned_merge(mf, size, tile, overlap, align):
    """n and status exact.  s, t within 1e-9 T relative: the bound of tests/test_align_gpu.py for one
    fit (fp64 sums in another order differ by <= n 2^-53 ~ 1e-12 relative, the det cancellation
    amplifies that by <= 12), once per step of the chain, since tile k's target is built from the
    coefficients before it.  The merged map within 2 fp32 ulp: one for the rounding (fma, as in the
    plain blend), one for a coefficient difference of <= 1e-8 relative flipping it.  The map the
    tiles were cut from comes back within twice the error of the reference on the same tiles."""
    D, tiles, (want, wcoef, _), diag = _case(size, tile, overlap, align)
    plan = _plan(mf, size, tile, overlap)
    x = torch.from_numpy(tiles.copy()).to(DEV)
    got, coef = mf.tile_merge(x[:, None], plan, size, align=align, max_depth=R.MAX_DEPTH)
    T = wcoef.shape[1]
    assert coef.shape == (B, T, 4) and coef.dtype == torch.float64
    coef_np, got_np = _np(coef), _np(got)[:, 0]
    assert np.array_equal(coef_np[..., 2:], wcoef[..., 2:])
    assert np.array_equal(coef_np[:, 0], wcoef[:, 0]) and wcoef[0, 0].tolist() == [1.0, 0.0, 0.0, 0.0]
    ymean = {(b, k): m for b, k, _, m in diag}
    worst = [0.0, 0.0]
    for b in range(B):
        for k in range(1, T):
            (s, t), (s_ref, t_ref) = coef_np[b, k, :2], wcoef[b, k, :2]
            ds, dt = abs(s - s_ref) / abs(s_ref), abs(t - t_ref) / (abs(t_ref) + ymean[(b, k)])
            worst = [max(worst[0], ds), max(worst[1], dt)]
            assert ds <= 1e-9 * T and dt <= 1e-9 * T, (b, k, s, s_ref, t, t_ref)
    d = R.ulp_diff(got_np, want)
    err, err_ref = np.abs(got_np - D).max(), np.abs(want - D).max()
    print(f"{align} {size}: T={T} worst ds {worst[0]:.2e} dt {worst[1]:.2e}; {int((d > 0).sum())} of {d.size} pixels "
          f"differ, max {d.max():.2f} ulp; recovery max|err| {err:.4e} (reference {err_ref:.4e})")
    assert d.max() <= 2
    assert err <= 2 * err_ref
    # two runs, an unaligned view and a strided input give the same bits
    for other in (x[:, None], _shifted(tiles), torch.stack([x, x], -1)[..., 0]):
        g2, c2 = mf.tile_merge(other, plan, size, align=align, max_depth=R.MAX_DEPTH)
        assert torch.equal(g2, got) and torch.equal(c2, coef)


@pytest.mark.parametrize("align", ALIGNS)
def test_failure_rule(mf, align):
    """The CPU test's cases: an overlap that is all NaN (n = 0), a constant tile (det = 0), a negative
    fitted scale; and a single pair.  The failed tile keeps s = 1, t = 0 and is blended as it is."""
    size, tile, overlap = (16, 40), (16, 24), (0, 8)
    plan = _plan(mf, size, tile, overlap)
    _, tiles = R.recoverable(size, tile, overlap, "lstsq", B=1, seed=1)
    t = tiles.copy()
    t[0, :, 16:] = np.nan
    c = tiles.copy()
    c[1] = 2.0
    n = tiles.copy()
    n[0] = 2.0 + np.arange(24, dtype=np.float32)[None, :] / 8
    n[1] = (6.0 - np.arange(24, dtype=np.float32)[None, :] / 8) if align == "lstsq" else n[0, :, ::-1]
    for name, x, cnt in (("nan", t, 0.0), ("const", c, 128.0), ("neg", n, 128.0)):
        got, coef = mf.tile_merge(torch.from_numpy(x.copy()).to(DEV), plan, size, align=align, max_depth=R.MAX_DEPTH)
        want, wcoef, _ = R.merge(x, size, tile, overlap, align, R.MAX_DEPTH)
        assert wcoef[0, 1].tolist() == [1.0, 0.0, cnt, 1.0], (name, wcoef)
        assert _np(coef)[0].tolist() == wcoef[0].tolist(), (name, _np(coef))
        assert R.ulp_diff(_np(got)[:, 0], want).max() <= 1, name
        if name == "nan":
            bad = np.isnan(_np(got)[0, 0])
            assert bad[:, 16:24].all() and not bad[:, :16].any() and not bad[:, 24:].any()
    plan1 = _plan(mf, (1, 7), (1, 4), (0, 1))
    _, coef = mf.tile_merge(torch.tensor([[[1., 2, 3, 4]], [[5, 6, 7, 8]]], device=DEV), plan1, (1, 7), align=align,
                            max_depth=R.MAX_DEPTH)
    assert _np(coef)[0, 1].tolist() == [1.0, 0.0, 1.0, 1.0]


@pytest.mark.parametrize("align", ("none",) + ALIGNS)
def test_a_nan_stays_where_its_tile_is(mf, align):
    """Image 0: tile 4 (the centre of the 3 x 3) all NaN -- the output is NaN on exactly the pixels
    that tile covers, every coefficient stays finite and the tile itself fails (n = 0).  Image 1:
    one NaN pixel, under one tile only -- exactly that pixel.  Two runs give the same bits."""
    size, tile, overlap = CASES[0]
    _, tiles, _, _ = _case(size, tile, overlap, align)
    plan = _plan(mf, size, tile, overlap)
    T = len(plan.ys) * len(plan.xs)
    x = tiles.copy()
    x[4] = np.nan
    x[T + 0, 2, 3] = np.nan  # image 1, tile 0, pixel (2, 3): no other tile reaches it
    run = lambda: mf.tile_merge(torch.from_numpy(x.copy()).to(DEV), plan, size, align=align, max_depth=R.MAX_DEPTH)
    got, coef = run()
    bad = np.isnan(_np(got)[:, 0])
    want = np.zeros((B,) + size, bool)
    want[0, plan.ys[1]:plan.ys[1] + tile[0], plan.xs[1]:plan.xs[1] + tile[1]] = True
    want[1, 2, 3] = True
    assert np.array_equal(bad, want)
    assert np.isfinite(_np(got)[:, 0][~want]).all()
    if align != "none":
        c = _np(coef)
        assert np.isfinite(c).all()
        assert c[0, 4].tolist() == [1.0, 0.0, 0.0, 1.0] and c[0, :, 3].sum() == 1 and not c[1, :, 3].any()
    got2, coef2 = run()
    assert torch.equal(got2.view(torch.int32), got.view(torch.int32))
    assert coef is None or torch.equal(coef2, coef)


def test_abi_refusals_launch_nothing(mf):
    """Every refused call returns MDEMI_EINVAL (a missing workspace: MDEMI_EWORKSPACE) with a message
    and leaves its outputs untouched."""
    from mdemi import _lib as L
    lib = L.load()
    H, W, th, tw = 40, 56, 24, 32
    img = torch.ones(1, 3, H, W, device=DEV)
    tiles = torch.ones(4, th, tw, device=DEV)
    out_t = torch.full((4, 3, th, tw), 7.0, device=DEV)
    out = torch.full((1, H, W), 7.0, device=DEV)
    coef = torch.full((1, 4, 4), 7.0, device=DEV, dtype=torch.float64)
    ws = torch.zeros(lib.mdemi_tile_align_workspace_size(1, th, tw), device=DEV, dtype=torch.uint8)
    assert ws.numel() >= 5 * 8

    def arr(*v):
        return (ctypes.c_int32 * len(v))(*v)

    good = (arr(0, 16), 2, arr(0, 24), 2)
    bad_plans = {"ny 0": (arr(0, 16), 0, arr(0, 24), 2), "nx 33": (arr(0, 16), 2, arr(*range(33)), 33),
                 "outside": (arr(0, 17), 2, arr(0, 24), 2), "negative": (arr(-1, 16), 2, arr(0, 24), 2),
                 "descending": (arr(16, 0), 2, arr(0, 24), 2), "equal": (arr(0, 16), 2, arr(24, 24), 2),
                 "null ys": (None, 2, arr(0, 24), 2)}
    s = L.stream()

    def extract(i=img.data_ptr(), o=out_t.data_ptr(), plan=good, th_=th):
        return lib.mdemi_tile_extract(i, o, 1, 3, H, W, th_, tw, *plan, s)

    def align(t=tiles.data_ptr(), c=coef.data_ptr(), plan=good, mode=L.ALIGN_LSTSQ, w=ws.data_ptr(), oy=8):
        return lib.mdemi_tile_align(t, 1, H, W, th, tw, oy, 8, *plan, mode, c, w, s)

    def blend(t=tiles.data_ptr(), c=None, o=out.data_ptr(), plan=good, mode=L.TILE_NONE, oy=8):
        return lib.mdemi_tile_blend(t, c, 1, H, W, th, tw, oy, 8, *plan, mode, 10.0, o, s)

    calls = [extract(i=None), extract(o=None), extract(i=img.data_ptr() + 2), extract(th_=H + 1),
             align(t=None), align(c=None), align(t=tiles.data_ptr() + 2), align(c=coef.data_ptr() + 4),
             align(mode=L.TILE_NONE), align(mode=L.ALIGN_MEDIAN), align(mode=7), align(oy=0), align(oy=th),
             align(w=ws.data_ptr() + 4),
             blend(t=None), blend(o=None), blend(o=out.data_ptr() + 2), blend(mode=L.ALIGN_MEDIAN), blend(mode=-1),
             blend(mode=L.ALIGN_LSTSQ), blend(oy=-1)]
    for name, plan in bad_plans.items():
        calls += [extract(plan=plan), align(plan=plan), blend(plan=plan)]
    calls += [align(plan=(arr(0, 10), 2, arr(0, 24), 2)), blend(plan=(arr(0, 16), 2, arr(0, 20), 2))]  # not to the border
    assert calls == [L.EINVAL] * len(calls), calls
    assert lib.mdemi_last_error().decode().startswith("tile_blend: ")
    assert align(w=None) == L.EWORKSPACE
    torch.cuda.synchronize()
    assert (out_t == 7).all() and (out == 7).all() and (coef == 7).all()
    # and the same arguments, unbroken, run
    assert extract() == 0 and align() == 0 and blend(c=coef.data_ptr(), mode=L.ALIGN_LSTSQ) == 0
    torch.cuda.synchronize()
    assert (out_t == 1).all() and (out == 1).all()
    assert _np(coef)[0, 0].tolist() == [1.0, 0.0, 0.0, 0.0] and (_np(coef)[0, 1:, 3] == 1).all()  # constant tiles
