"""The fp64 reference of the GEMM descriptor contract (tests/gemm_contract_ref.py) against
torch's own operators, and the exactness of every exact-regime case of
tests/gemm_contract_cases.py -- what entitles tests/test_gemm_contract_gpu.py to torch.equal.
CPU only."""
import pytest
import torch
import torch.nn.functional as F

import gemm_contract_cases as G
import gemm_contract_ref as R


def dense(d, name, rows, cols, ld, b=0, bstride=0):
    """[rows, cols] of a row-major tensor by plain slicing (not through gemm_contract_ref)."""
    buf, off = getattr(d, name), getattr(d, name + "_off") + b * bstride
    return buf[off:off + rows * ld].view(rows, ld)[:, :cols].double()


@pytest.mark.parametrize("aligned", [True, False])
def test_linear_matches_F_linear(aligned):
    """k-contiguous A and B with a column bias is nn.Linear: C = x W^T + b."""
    c = G.Case(name="linear", M=37, N=21, K=50, bias_mode=R.BIAS_COL, aligned=aligned, seed=1)
    d = G.build(c)
    x, w = dense(d, "A", c.M, c.K, d.lda), dense(d, "B", c.N, c.K, d.ldb)
    bias = d.bias[d.bias_off:d.bias_off + c.N].double()
    assert not torch.isnan(x).any() and d.lda > c.K and d.ldb > c.K and d.ldc > c.N
    assert torch.equal(R.operand(d, "A")[0], x) and torch.equal(R.operand(d, "B")[0], w.t())
    assert torch.equal(R.expected(d).C[0], F.linear(x, w, bias))


@pytest.mark.parametrize("pair", list(G.LAYOUT_PAIRS))
def test_layouts_and_batches_match_einsum(pair):
    """All four dense layout pairs, batch 3 with batch strides (and a broadcast A), against
    torch.einsum on plainly sliced storage."""
    al, bl = G.LAYOUT_PAIRS[pair]
    for bcast in (False, True):
        c = G.Case(name="einsum", M=19, N=23, K=11, batch=3, a_layout=al, b_layout=bl, a_broadcast=bcast,
                   aligned=not bcast, seed=2)
        d = G.build(c)
        assert (d.a_bstride == 0) == bcast and d.b_bstride > (c.K if bl == R.L_MNCONTIG else c.N) * d.ldb
        a = torch.stack([dense(d, "A", c.M, c.K, d.lda, b, d.a_bstride) if al == R.L_KCONTIG
                         else dense(d, "A", c.K, c.M, d.lda, b, d.a_bstride).t() for b in range(3)])
        bm = torch.stack([dense(d, "B", c.N, c.K, d.ldb, b, d.b_bstride).t() if bl == R.L_KCONTIG
                          else dense(d, "B", c.K, c.N, d.ldb, b, d.b_bstride) for b in range(3)])
        assert torch.equal(R.expected(d).C, torch.einsum("bik,bkj->bij", a, bm))


def test_batch_inner_is_heads_as_column_slices():
    """batch_inner: z = o * batch_inner + i reads columns [i K, (i + 1) K) of image o's token
    rows -- against einsum over the [outer, rows, heads, K] view."""
    c = G.Case(name="inner", M=9, N=5, K=8, batch=6, batch_inner=3, b_layout=R.L_MNCONTIG, seed=3)
    d = G.build(c)
    a = torch.stack([dense(d, "A", c.M, 3 * c.K, d.lda, o, d.a_bstride).view(c.M, 3, c.K) for o in range(2)])
    b = torch.stack([dense(d, "B", c.K, 3 * c.N, d.ldb, o, d.b_bstride).view(c.K, 3, c.N) for o in range(2)])
    want = torch.einsum("omhk,okhn->ohmn", a, b).reshape(6, c.M, c.N)
    assert torch.equal(R.expected(d).C, want)


def _pad_or_crop(x, top, bottom, left, right, mode):
    """x [n, c, h, w]: negative amounts crop, positive ones pad (zero or replicate)."""
    h, w = x.shape[2:]
    x = x[:, :, max(-top, 0):h - max(-bottom, 0), max(-left, 0):w - max(-right, 0)]
    pads = (max(left, 0), max(right, 0), max(top, 0), max(bottom, 0))
    return F.pad(x, pads, mode="replicate") if mode == R.PAD_REPLICATE else F.pad(x, pads)


@pytest.mark.parametrize("name,cv", G._geometries(4) + G._geometries(12), ids=lambda v: v if isinstance(v, str) else "")
def test_im2col_matches_conv2d(name, cv):
    """The explicit im2col matrix times the flattened filter is F.conv2d on the explicitly padded
    (F.pad, zero or replicate) or cropped input: stride, negative pad, TF-'same' bottom/right
    padding from oh / ow -- as operand A, and as operand B (the weight gradient)."""
    case = G.Case(name=name, M=cv.n * cv.oh * cv.ow, N=6, K=cv.kh * cv.kw * cv.c, a_layout=R.L_CONV, conv=cv, seed=4)
    d = G.build(case)
    x = d.A[d.A_off:d.A_off + cv.n * cv.h * cv.w * cv.c].view(cv.n, cv.h, cv.w, cv.c).double()
    w = dense(d, "B", 6, case.K, d.ldb).view(6, cv.kh, cv.kw, cv.c)
    bottom = (cv.oh - 1) * cv.stride + cv.kh - cv.h - cv.pad
    right = (cv.ow - 1) * cv.stride + cv.kw - cv.w - cv.pad
    xp = _pad_or_crop(x.permute(0, 3, 1, 2), cv.pad, bottom, cv.pad, right, cv.pad_mode)
    y = F.conv2d(xp, w.permute(0, 3, 1, 2), stride=cv.stride)
    assert y.shape[2:] == (cv.oh, cv.ow)
    assert torch.equal(R.expected(d).C[0], y.permute(0, 2, 3, 1).reshape(case.M, 6))
    # the weight gradient dW[o, (ky, kx, c)] = sum_pixels dY[pixel, o] * im2col[pixel, (ky, kx, c)]
    wg = G.Case(name=name, M=6, N=case.K, K=case.M, a_layout=R.L_MNCONTIG, b_layout=R.L_CONV, conv=cv, rowsum=True, seed=5)
    dg = G.build(wg)
    dy = dense(dg, "A", wg.K, 6, dg.lda)
    xg = dg.B[dg.B_off:dg.B_off + cv.n * cv.h * cv.w * cv.c].view(cv.n, cv.h, cv.w, cv.c).double()
    xpg = _pad_or_crop(xg.permute(0, 3, 1, 2), cv.pad, bottom, cv.pad, right, cv.pad_mode).requires_grad_()
    wz = torch.zeros(6, cv.c, cv.kh, cv.kw, dtype=torch.float64, requires_grad=True)
    F.conv2d(xpg, wz, stride=cv.stride).backward(dy.view(cv.n, cv.oh, cv.ow, 6).permute(0, 3, 1, 2))
    out = R.expected(dg)
    assert torch.equal(out.C[0], wz.grad.permute(0, 2, 3, 1).reshape(6, wg.N))
    assert torch.equal(out.rowsum_a, dy.sum(0))


def test_epilogue_stage_order():
    """alpha, beta, bias, preact, activation, row_scale, residual in the header's order, against
    the formula written out with torch's activations; the gradient activations against autograd."""
    acts = {R.ACT_NONE: lambda v: v, R.ACT_GELU: F.gelu, R.ACT_RELU: F.relu, R.ACT_SIGMOID: torch.sigmoid,
            R.ACT_SILU: F.silu, R.ACT_LEAKY: lambda v: F.leaky_relu(v, R.LEAKY_SLOPE)}
    grads = {R.ACT_GELU_GRAD: F.gelu, R.ACT_RELU_GRAD: F.relu, R.ACT_SILU_GRAD: F.silu}
    for i, act in enumerate(list(acts) + list(grads)):
        c = G.Case(name="stages", M=13, N=9, K=6, alpha=0.5, beta=0.25, bias_mode=(R.BIAS_COL, R.BIAS_ROW)[i % 2], act=act,
                   preact=True, residual=True, row_scale_group=4, regime="smooth", aligned=i % 2 == 0, seed=6 + i)
        d = G.build(c)
        a, b = dense(d, "A", c.M, c.K, d.lda), dense(d, "B", c.N, c.K, d.ldb)
        c0, res = dense(d, "C", c.M, c.N, d.ldc), dense(d, "residual", c.M, c.N, d.ldres)
        n = c.N if c.bias_mode == R.BIAS_COL else c.M
        bias = d.bias[d.bias_off:d.bias_off + n].double()
        rs = d.row_scale[d.row_scale_off:d.row_scale_off + 4].double().repeat_interleave(4)[:c.M, None]
        pre = 0.5 * (a @ b.t()) + 0.25 * c0 + (bias[None, :] if c.bias_mode == R.BIAS_COL else bias[:, None])
        if act in grads:
            aux = dense(d, "aux", c.M, c.N, d.ldaux).requires_grad_()
            grads[act](aux).sum().backward()
            mid = pre * aux.grad
        else:
            mid = acts[act](pre)
        out = R.expected(d, round32=False)
        assert torch.equal(out.preact[0], pre)
        torch.testing.assert_close(out.C[0], mid * rs + res, rtol=1e-13, atol=1e-13)
    assert R.LEAKY_SLOPE == float(torch.tensor(0.01, dtype=torch.float32)) != 0.01


@pytest.mark.parametrize("case", G.exact_cases(), ids=lambda c: c.name)
def test_exact_cases_are_exact(case):
    """Every case held to torch.equal on the GPU: K <= 2112, operands that are bf16 numbers, and
    every partial sum and epilogue stage an fp32 number (LEAKY: up to its one rounded multiply and
    the row_scale multiply after it, and then no residual, whose add could fuse with it)."""
    d = G.build(case)
    out = R.expected(d)
    assert case.K <= 2112
    for which in "AB":
        x = R.operand(d, which)
        assert torch.equal(x.bfloat16().double(), x)
    if case.act == R.ACT_LEAKY:
        assert set(out.inexact) <= {"act", "row_scale"} and not case.residual, out.inexact
    else:
        assert out.inexact == [], out.inexact
    # rounding per stage changed nothing, so the unrounded fp64 evaluation is the same number
    if not out.inexact:
        assert torch.equal(R.expected(d, round32=False).C, out.C)
    # guard bands: every tensor's leading dimension exceeds its extent and slack follows it
    for name, mask in d.masks.items():
        buf = getattr(d, name)
        assert mask.sum().item() < buf.numel() - G.SLACK_ROWS
        assert (buf.view(torch.int32)[~mask] == G.PATTERN).all()


def test_smooth_cases_have_exact_preactivations():
    """Smooth epilogue cases: alpha * acc + bias is exact and spans about [-8, 8]."""
    for case in G.smooth_epilogue_cases():
        d = G.build(case)
        out = R.expected(d, round32=False)
        assert not {"acc", "partial sums", "alpha", "beta", "bias"} & set(out.inexact), (case.name, out.inexact)
        q = out.preact.abs().flatten().quantile(0.95).item()
        assert 4.0 <= q <= 16.0, (case.name, q)
    for case in G.gelu_load_cases():
        assert case.K <= 128 and case.act == R.ACT_NONE
