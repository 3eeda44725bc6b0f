"""fp64 CPU statement of the GEMM descriptor contract (mdemi_gemm_desc in include/mdemi.h),
written from the header's wording in plain torch.  Nothing of the library is imported: the
constants below restate the header's #defines.

A "descriptor" here is any object with the header's field names whose pointer fields
(A, B, C, bias, aux, residual, preact, rowsum_a, row_scale) are 1-D CPU tensors -- the whole
allocation the pointer points into -- each with an element offset `<name>_off` of the pointer
from the start of that allocation.  Every element is read through torch.as_strided on that
allocation, which refuses a view that leaves it: a reference that can be computed at all has
proved that the descriptor's extents lie inside the buffers it names.

  operand(d, "A") -> A[b, i, k]      operand(d, "B") -> B[b, k, j]
  expected(d)     -> C, preact, rowsum_a after the epilogue stages in the header's order
"""
import math
from types import SimpleNamespace

import torch

L_KCONTIG, L_MNCONTIG, L_CONV = 0, 1, 2
OP_NONE, OP_GELU = 0, 1
BIAS_NONE, BIAS_COL, BIAS_ROW = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_RELU, ACT_LEAKY, ACT_GELU_GRAD, ACT_SIGMOID = 0, 1, 2, 3, 4, 5
ACT_SILU, ACT_RELU_GRAD, ACT_SILU_GRAD = 6, 7, 8
GRAD_ACTS = (ACT_GELU_GRAD, ACT_RELU_GRAD, ACT_SILU_GRAD)
PAD_ZERO, PAD_REPLICATE = 0, 1


def f32c(c):
    """An fp32 constant of the contract as the double it is: double(float32(c))."""
    return torch.tensor(float(c), dtype=torch.float32).double().item()


LEAKY_SLOPE = f32c(0.01)  # MDEMI_ACT_LEAKY: negative slope 0.01 (nn.LeakyReLU default)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def silu_grad(x):
    s = sigmoid(x)
    return s + x * s * (1.0 - s)


def batch_offsets(d, stride, stride_inner=0):
    """Element offset of every batch entry z: z * stride, or with batch_inner > 1
    (z = o * batch_inner + i) o * stride + i * stride_inner."""
    bi = getattr(d, "batch_inner", 0)
    if bi > 1:
        return [(z // bi) * stride + (z % bi) * stride_inner for z in range(d.batch)]
    return [z * stride for z in range(d.batch)]


def strided(buf, off, rows, cols, row_stride, col_stride):
    """[rows, cols] of allocation `buf` as float64; raises if any element lies outside it."""
    return torch.as_strided(buf, (rows, cols), (row_stride, col_stride), off).double()


def matrices(d, name, rows, cols, ld, bstride, bstride_inner=0):
    """[batch, rows, cols] of the row-major tensor `name` (C, aux, residual, preact)."""
    buf, off = getattr(d, name), getattr(d, name + "_off", 0)
    return torch.stack([strided(buf, off + o, rows, cols, ld, 1) for o in batch_offsets(d, bstride, bstride_inner)])


def im2col(x, g):
    """Explicit im2col matrix [n * oh * ow, kh * kw * c] of the NHWC activation x [n, h, w, c]
    under mdemi_conv_geom g: input row of output row oy and tap ky is oy * stride - pad + ky
    (pad may be negative, a crop); rows / columns outside [0, h) / [0, w) -- on any side, the
    bottom / right ones following from oh / ow -- read 0 (MDEMI_PAD_ZERO) or the nearest edge
    pixel (MDEMI_PAD_REPLICATE)."""
    iy = torch.arange(g.oh)[:, None] * g.stride - g.pad + torch.arange(g.kh)[None, :]  # [oh, kh]
    ix = torch.arange(g.ow)[:, None] * g.stride - g.pad + torch.arange(g.kw)[None, :]  # [ow, kw]
    vy, vx = (iy >= 0) & (iy < g.h), (ix >= 0) & (ix < g.w)
    iy, ix = iy.clamp(0, g.h - 1), ix.clamp(0, g.w - 1)
    t = x[:, iy]                # [n, oh, kh, w, c]
    t = t[:, :, :, ix]          # [n, oh, kh, ow, kw, c]
    t = t.permute(0, 1, 3, 2, 4, 5)  # [n, oh, ow, kh, kw, c]
    if g.pad_mode == PAD_ZERO:
        inside = vy[:, None, :, None] & vx[None, :, None, :]  # [oh, ow, kh, kw]
        t = torch.where(inside[None, :, :, :, :, None], t, torch.zeros((), dtype=t.dtype))
    return t.reshape(g.n * g.oh * g.ow, g.kh * g.kw * g.c)


def operand(d, which):
    """The logical operand of descriptor d: A[b, i, k] ("A") or B[b, k, j] ("B"), float64,
    read through its layout, leading dimension, batch strides and load-time op."""
    a = which == "A"
    buf, off = (d.A, getattr(d, "A_off", 0)) if a else (d.B, getattr(d, "B_off", 0))
    layout, ld, op = (d.a_layout, d.lda, d.a_op) if a else (d.b_layout, d.ldb, d.b_op)
    bs = d.a_bstride if a else d.b_bstride
    bs2 = getattr(d, "a_bstride_inner" if a else "b_bstride_inner", 0)
    ext = d.M if a else d.N  # the non-reduction extent
    out = []
    for o in batch_offsets(d, bs, bs2):
        if layout == L_CONV:
            g = d.conv
            x = strided(buf, off + o, g.n * g.h * g.w, g.c, g.c, 1).reshape(g.n, g.h, g.w, g.c)
            m = im2col(x, g)  # [pixels, taps]: A(i = pixel, k = tap) and B(k = pixel, j = tap) alike
            assert m.shape == ((d.M, d.K) if a else (d.K, d.N)), "conv operand: M/N/K do not match the geometry"
        elif layout == L_KCONTIG:  # A stored [i][k]; B stored [j][k]
            m = strided(buf, off + o, ext, d.K, ld, 1)
            m = m if a else m.t()
        else:                      # A stored [k][i]; B stored [k][j]
            m = strided(buf, off + o, d.K, ext, ld, 1)
            m = m.t() if a else m
        out.append(gelu(m) if op == OP_GELU else m)
    return torch.stack(out)


def _act(act, v, aux):
    if act == ACT_NONE:
        return v
    if act == ACT_GELU:
        return gelu(v)
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, LEAKY_SLOPE * v)
    if act == ACT_SIGMOID:
        return sigmoid(v)
    if act == ACT_SILU:
        return v * sigmoid(v)
    if act == ACT_GELU_GRAD:
        return v * gelu_grad(aux)
    if act == ACT_RELU_GRAD:
        return v * (aux > 0).double()
    if act == ACT_SILU_GRAD:
        return v * silu_grad(aux)
    raise ValueError(f"unknown activation {act}")


def expected(d, round32=True):
    """The outputs of descriptor d, float64, stage by stage in the header's order:
      1 alpha * acc   2 + beta * C0   3 + bias   4 store preact   5 act (or * act'(aux))
      6 * row_scale[i / group]   7 + residual
    round32: every stage is rounded to fp32 before the next one -- an fp32 evaluation with
    one rounding per stage.  Returns C [batch, M, N], preact (or None), rowsum_a [M] (or None),
    `stages` (name -> value before rounding) and `inexact`: the stages whose value was not
    already an fp32 number (empty: every summation order, split and fused multiply-add must
    reproduce C bit for bit)."""
    A, B = operand(d, "A"), operand(d, "B")
    stages, inexact = {}, []

    def stage(name, v):
        stages[name] = v
        r = v.float().double()
        if not torch.equal(r, v):
            inexact.append(name)
        return r if round32 else v

    v = stage("acc", torch.bmm(A.contiguous(), B.contiguous()))
    # every partial sum is exact when the sum of the magnitudes is: no order can round
    mag = torch.bmm(A.abs().contiguous(), B.abs().contiguous())
    if not torch.equal(mag.float().double(), mag) or mag.max().item() >= 2.0 ** 24 * _ulp_unit(A, B):
        inexact.append("partial sums")
    v = stage("alpha", f32c(d.alpha) * v)
    bs2 = getattr(d, "c_bstride_inner", 0)
    if d.beta != 0.0:
        v = stage("beta", v + f32c(d.beta) * matrices(d, "C", d.M, d.N, d.ldc, d.c_bstride, bs2))
    if d.bias_mode != BIAS_NONE:
        n = d.N if d.bias_mode == BIAS_COL else d.M
        bias = strided(d.bias, getattr(d, "bias_off", 0), 1, n, n, 1)[0]
        v = stage("bias", v + (bias[None, None, :] if d.bias_mode == BIAS_COL else bias[None, :, None]))
    pre = v.clone() if getattr(d, "preact", None) is not None else None
    if d.act != ACT_NONE:
        aux = matrices(d, "aux", d.M, d.N, d.ldaux, d.aux_bstride) if d.act in GRAD_ACTS else None
        v = stage("act", _act(d.act, v, aux))
    if getattr(d, "row_scale", None) is not None:
        groups = (d.M + d.row_scale_group - 1) // d.row_scale_group
        rs = strided(d.row_scale, getattr(d, "row_scale_off", 0), 1, groups, groups, 1)[0]
        v = stage("row_scale", v * rs[torch.arange(d.M) // d.row_scale_group][None, :, None])
    if getattr(d, "residual", None) is not None:
        v = stage("residual", v + matrices(d, "residual", d.M, d.N, d.ldres, d.res_bstride))
    rowsum = None
    if getattr(d, "rowsum_a", None) is not None:
        rowsum = stage("rowsum_a", A[0].sum(1))
        rmag = A[0].abs().sum(1)
        if not torch.equal(rmag.float().double(), rmag):
            inexact.append("rowsum_a partial sums")
    return SimpleNamespace(C=v, preact=pre, rowsum_a=rowsum, stages=stages, inexact=inexact)


def _ulp_unit(A, B):
    """Smallest power of two that every product a * b is a multiple of (1 for integers): a sum
    of such products below 2^24 units has every partial sum exact in fp32."""
    unit = 1.0
    for t in (A, B):
        u = 1.0
        while u > 2.0 ** -30 and not torch.equal((t / u).round(), t / u):
            u /= 2.0
        unit *= u
    return unit
