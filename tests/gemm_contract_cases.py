"""Cases, guard-banded buffers and comparison helpers of the GEMM descriptor contract tests
(tests/test_gemm_contract_ref.py on the CPU, tests/test_gemm_contract_gpu.py on the GPU).
Plain torch on the CPU; nothing of the library is imported.

build(case) lays every tensor of one descriptor out inside a larger allocation of its own:
an element offset before it, a leading dimension larger than the extent, a batch stride
larger than rows * ld and SLACK_ROWS rows after the last one.  Input slack is NaN -- a read
past an extent poisons the result -- and output slack, and C itself when beta == 0, holds
PATTERN, a quiet NaN with a recognisable payload: a write past an extent changes a slack
word, an element never written stays NaN, and a beta == 0 call that reads C produces NaN.

Exact regime: operands are integers in [-4, 4], alpha in {1, 0.5, -2}, beta in {0, 0.25} on
an integer C0, bias integers / 8, residual integers / 4, row_scale in {0, 1.25, 2}, K <= 2112.
Every partial sum (|acc| <= 16 K < 2^24) and every epilogue stage is then an fp32 number, so
no summation order, K split, combine path or fused multiply-add can change a bit, and the
operands are bf16 numbers too.  MDEMI_ACT_LEAKY adds one correctly rounded multiply; a LEAKY
case takes no residual, because `slope * v + residual` may be evaluated with one rounding
(fused) or two.  expected(...).inexact states which stages were not exact; the CPU test holds
every exact case to it.
"""
from dataclasses import dataclass, replace
from types import SimpleNamespace

import torch

import gemm_contract_ref as R

SLACK_ROWS = 256           # one block tile of the tallest variant
PATTERN = 0x7FC0BEEF       # int32 view of the output fill: a quiet NaN


@dataclass(frozen=True)
class Conv:
    n: int
    h: int
    w: int
    c: int
    oh: int
    ow: int
    kh: int
    kw: int
    stride: int
    pad: int
    pad_mode: int


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    a_layout: int = R.L_KCONTIG
    b_layout: int = R.L_KCONTIG
    a_op: int = R.OP_NONE
    b_op: int = R.OP_NONE
    batch: int = 1
    batch_inner: int = 0      # > 1: heads as column slices of the token buffers
    a_broadcast: bool = False  # a_bstride = 0
    alpha: float = 1.0
    beta: float = 0.0
    bias_mode: int = R.BIAS_NONE
    act: int = R.ACT_NONE
    preact: bool = False
    residual: bool = False
    row_scale_group: int = 0  # > 0: row_scale over groups of this many rows
    rowsum: bool = False
    split_k: int = 1
    conv: Conv = None
    aligned: bool = True
    dense_c: bool = False     # ldc == N (what the deep split-K combine needs)
    regime: str = "exact"     # or "smooth"
    seed: int = 0


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


class _Layout:
    """Offsets, leading dimensions and batch strides of one alignment form.
    aligned: 16-B aligned bases, ld % 4 == 0, strides % 4 == 0 (vector loads and the DMA variants
    run as themselves where the extents allow); else odd offsets, leading dimensions and strides
    (scalar loaders; forced DMA variants fall back)."""

    def __init__(self, aligned):
        self.aligned = aligned

    def off(self):
        return 8 if self.aligned else 5

    def ld(self, extent):
        if self.aligned:
            return (extent + 3) // 4 * 4 + 4
        return extent + 1 if extent % 2 == 0 else extent + 2

    def bstride(self, rows, ld):
        s = (rows + 3) * ld
        if self.aligned:
            return (s + 3) // 4 * 4 + 4
        return s + 1 if s % 2 == 0 else s + 2


def _alloc(n, output):
    if output:
        return torch.full((n,), PATTERN, dtype=torch.int32).view(torch.float32).clone()
    return torch.full((n,), float("nan"), dtype=torch.float32)


def _place(values, off, ld, offsets, output=False, fill=True):
    """values [nb, rows, cols] laid out row-major with leading dimension ld at element offsets
    off + offsets[b] of a fresh allocation; returns (allocation, mask of the logical elements).
    An output that the call only writes keeps PATTERN in its logical elements (fill=False)."""
    nb, rows, cols = values.shape
    n = off + max(offsets) + (rows + SLACK_ROWS) * ld
    buf, mask = _alloc(n, output), torch.zeros(n, dtype=torch.bool)
    for b, o in enumerate(offsets):
        torch.as_strided(mask, (rows, cols), (ld, 1), off + o).fill_(True)
        if fill:
            torch.as_strided(buf, (rows, cols), (ld, 1), off + o).copy_(values[b].float())
    return buf, mask


def _vector(values, off, output=False, fill=True):
    buf, mask = _place(values.reshape(1, 1, -1), off, values.numel(), [0], output, fill)
    return buf, mask


def build(case):
    """The descriptor of `case` for gemm_contract_ref (CPU allocations, element offsets) with
    d.masks[name]: the logical elements of every output allocation."""
    c, g = case, torch.Generator().manual_seed(1000 + case.seed)
    lay = _Layout(c.aligned)
    d = SimpleNamespace(M=c.M, N=c.N, K=c.K, batch=c.batch, batch_inner=c.batch_inner, a_layout=c.a_layout,
                        b_layout=c.b_layout, a_op=c.a_op, b_op=c.b_op, alpha=c.alpha, beta=c.beta,
                        bias_mode=c.bias_mode, act=c.act, split_k=c.split_k, conv=c.conv, masks={}, case=c,
                        a_bstride_inner=0, b_bstride_inner=0, c_bstride_inner=0, bias=None, aux=None, residual=None,
                        preact=None, rowsum_a=None, row_scale=None, row_scale_group=0, ldaux=0, aux_bstride=0,
                        ldres=0, res_bstride=0, ldpre=0, pre_bstride=0)
    nb, heads = c.batch, max(c.batch_inner, 1)
    smooth_load = c.a_op == R.OP_GELU or c.b_op == R.OP_GELU

    def operand(which):
        layout = c.a_layout if which == "A" else c.b_layout
        ext = c.M if which == "A" else c.N
        gelu_in = (c.a_op if which == "A" else c.b_op) == R.OP_GELU
        if layout == R.L_CONV:  # a dense NHWC activation, 16-B aligned, no leading dimension
            cv = c.conv
            x = _ints(g, -4, 4, 1, cv.n * cv.h * cv.w, cv.c)
            buf, _ = _place(x, 8, cv.c, [0])
            return buf, 8, cv.c, 0, 0
        rows, cols = (ext, c.K) if layout == R.L_KCONTIG else (c.K, ext)
        bcast = which == "A" and c.a_broadcast
        nvals = 1 if bcast else nb
        vals = _ints(g, -32, 32, nvals, rows, cols) / 8 if gelu_in else _ints(g, -4, 4, nvals, rows, cols)
        if heads > 1:  # head i is a column slice of the [rows][heads * cols] buffer of image o
            ld = lay.ld(heads * cols)
            bs, bs2 = lay.bstride(rows, ld), cols
            offs = R.batch_offsets(SimpleNamespace(batch=nb, batch_inner=heads), bs, bs2)
        else:
            ld = lay.ld(cols)
            bs, bs2 = (0 if bcast else lay.bstride(rows, ld)), 0
            offs = [0] if bcast else [z * bs for z in range(nb)]
        buf, _ = _place(vals, lay.off(), ld, offs)
        return buf, lay.off(), ld, bs, bs2

    d.A, d.A_off, d.lda, d.a_bstride, d.a_bstride_inner = operand("A")
    d.B, d.B_off, d.ldb, d.b_bstride, d.b_bstride_inner = operand("B")

    def matrix(name, values, output=False, fill=True, dense=False):
        if heads > 1:
            ld = lay.ld(heads * c.N)
            bs, bs2 = lay.bstride(c.M, ld), c.N
            offs = R.batch_offsets(SimpleNamespace(batch=nb, batch_inner=heads), bs, bs2)
        else:
            ld = c.N if dense else lay.ld(c.N)
            bs, bs2 = lay.bstride(c.M, ld), 0
            offs = [z * bs for z in range(nb)]
        buf, mask = _place(values, lay.off(), ld, offs, output, fill)
        if output:
            d.masks[name] = mask
        return buf, lay.off(), ld, bs, bs2

    c0 = _ints(g, -8, 8, nb, c.M, c.N)
    d.C, d.C_off, d.ldc, d.c_bstride, d.c_bstride_inner = matrix("C", c0, output=True, fill=c.beta != 0.0,
                                                                 dense=c.dense_c)
    if c.bias_mode != R.BIAS_NONE:
        n = c.N if c.bias_mode == R.BIAS_COL else c.M
        d.bias_off = 4 if c.aligned else 1
        d.bias, _ = _vector(_ints(g, -16, 16, n) / 8, d.bias_off)
    if c.act in R.GRAD_ACTS:
        aux = _ints(g, -4, 4, nb, c.M, c.N) if c.regime == "exact" else _ints(g, -32, 32, nb, c.M, c.N) / 8
        d.aux, d.aux_off, d.ldaux, d.aux_bstride, _ = matrix("aux", aux)
    if c.residual:
        d.residual, d.residual_off, d.ldres, d.res_bstride, _ = matrix("residual", _ints(g, -16, 16, nb, c.M, c.N) / 4)
    if c.preact:
        d.preact, d.preact_off, d.ldpre, d.pre_bstride, _ = matrix("preact", c0, output=True, fill=False)
    if c.row_scale_group:
        groups = (c.M + c.row_scale_group - 1) // c.row_scale_group
        scale = torch.tensor([0.0, 1.25, 2.0], dtype=torch.float64)[torch.randint(0, 3, (groups,), generator=g)]
        d.row_scale_group, d.row_scale_off = c.row_scale_group, (4 if c.aligned else 3)
        d.row_scale, _ = _vector(scale, d.row_scale_off)
    if c.rowsum:
        d.rowsum_a_off = 4 if c.aligned else 1
        d.rowsum_a, d.masks["rowsum_a"] = _vector(torch.zeros(c.M), d.rowsum_a_off, output=True, fill=False)
    assert not (smooth_load and c.regime == "exact")
    return d


OUTPUTS = ("C", "preact", "rowsum_a")


def logical(d, name, buf):
    """The logical elements of output `name` read from allocation `buf` (d's layout), shaped as
    gemm_contract_ref.expected returns them; `buf` may live on any device."""
    off = getattr(d, name + "_off")
    if name == "rowsum_a":
        return buf[off:off + d.M]
    ld, bs, bs2 = (d.ldc, d.c_bstride, d.c_bstride_inner) if name == "C" else (d.ldpre, d.pre_bstride, 0)
    return torch.stack([torch.as_strided(buf, (d.M, d.N), (ld, 1), off + o) for o in R.batch_offsets(d, bs, bs2)])


def slack_damage(buf, mask):
    """Indices of the slack words of an output allocation that no longer hold PATTERN."""
    bad = (buf.view(torch.int32) != PATTERN) & ~mask.to(buf.device)
    return bad.nonzero().flatten().tolist()


def check_exact(got, want32, what):
    """got == want32 bit for bit as numbers (torch.equal), with the first mismatch in the message."""
    assert not torch.isnan(got).any().item(), f"{what}: NaN in the output (unwritten element or a read of slack)"
    if not torch.equal(got, want32):
        bad = (got != want32).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ from the fp64 reference "
                             f"rounded to fp32; first at {i}: got {got[i].item()!r}, want {want32[i].item()!r}")


def check_close(got, want, bound, what):
    """|got - want| <= bound per element (want, bound float64)."""
    assert not torch.isnan(got).any().item(), f"{what}: NaN in the output (unwritten element or a read of slack)"
    err = (got.double() - want).abs()
    if not (err <= bound).all().item():
        bad = (err > bound).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements out of tolerance; first at {i}: "
                             f"got {got[i].item()!r}, want {want[i].item()!r}, |err| {err[i].item():.3e} > "
                             f"{bound[i].item():.3e}")


def check_slack(buf, mask, what):
    bad = slack_damage(buf, mask)
    assert not bad, f"{what}: {len(bad)} slack words overwritten, first at element {bad[0]}"


# ---------------------------------------------------------------------------------------------
# The cases
# ---------------------------------------------------------------------------------------------
K_, MN_, CV_ = R.L_KCONTIG, R.L_MNCONTIG, R.L_CONV
LAYOUT_PAIRS = {"k_k": (K_, K_), "k_mn": (K_, MN_), "mn_k": (MN_, K_), "mn_mn": (MN_, MN_)}

# Full epilogues of the exact regime (every stage exact; LEAKY: no residual, see the module text)
EPILOGUES = [
    dict(alpha=0.5, beta=0.25, bias_mode=R.BIAS_COL, preact=True, act=R.ACT_RELU, row_scale_group=48, residual=True),
    dict(alpha=-2.0, beta=0.0, bias_mode=R.BIAS_ROW, preact=True, act=R.ACT_LEAKY, row_scale_group=100),
    dict(alpha=1.0, beta=0.25, bias_mode=R.BIAS_COL, preact=True, act=R.ACT_RELU_GRAD, row_scale_group=7,
         residual=True),
    dict(alpha=-2.0, beta=0.0, bias_mode=R.BIAS_ROW, preact=True, act=R.ACT_NONE, residual=True),
]

# The smallest shapes that straddle what the kernels tile by: 128- / 256-row tiles, 128- / 192-
# column tiles, BK 16 / 32, the 32-element split chunk.
SHAPES = [(1, 1, 1), (128, 128, 32), (129, 130, 33), (257, 193, 70), (256, 192, 64), (300, 200, 100), (64, 64, 31),
          (64, 64, 32), (64, 64, 33)]


def _both(case):
    return [replace(case, name=case.name + "-aligned", aligned=True),
            replace(case, name=case.name + "-misaligned", aligned=False, seed=case.seed + 500)]


def shape_cases(shape, pair):
    """One shape in one layout pair, a full epilogue, aligned and misaligned; rowsum_a wherever A
    is m-contiguous."""
    M, N, K = shape
    al, bl = LAYOUT_PAIRS[pair]
    si, li = SHAPES.index(shape), list(LAYOUT_PAIRS).index(pair)
    ep = EPILOGUES[(si + li) % len(EPILOGUES)]
    return _both(Case(name=f"{M}x{N}x{K}-{pair}", M=M, N=N, K=K, a_layout=al, b_layout=bl, rowsum=al == MN_,
                      seed=10 * si + li, **ep))


def combine_cases():
    """Split-K over a full epilogue: split_k 1, 3, 7 and more pieces than K chunks (300 = 10
    chunks), N % 4 == 0 (the reduce kernel's 16-B path) and N % 4 != 0."""
    out = []
    for ni, N in enumerate((132, 130)):
        for si, split in enumerate((1, 3, 7, 16)):
            ep = EPILOGUES[(ni + si) % len(EPILOGUES)]
            al, bl = ((K_, K_), (MN_, MN_), (K_, MN_), (MN_, K_))[si]
            out += _both(Case(name=f"split{split}-N{N}", M=129, N=N, K=300, a_layout=al, b_layout=bl,
                              rowsum=al == MN_, split_k=split, seed=100 + 10 * ni + si, **ep))
    return out


def deep_cases():
    """split_k = 33 at (24, 40, 1056): 33 chunks, the deep column-sum combine when ldc == N and
    the epilogue is a plain store; the same split with ldc > N, with row_scale, with rowsum_a."""
    base = Case(name="deep", M=24, N=40, K=1056, a_layout=MN_, b_layout=MN_, split_k=33, dense_c=True, seed=200)
    return (_both(replace(base, name="deep-plain"))
            + _both(replace(base, name="deep-ldc", dense_c=False, seed=201))
            + _both(replace(base, name="deep-row_scale", row_scale_group=5, seed=202))
            + _both(replace(base, name="deep-rowsum", rowsum=True, seed=203)))


def batch_cases():
    base = Case(name="batch3", M=130, N=36, K=70, batch=3, alpha=0.5, beta=0.25, bias_mode=R.BIAS_COL, seed=300)
    grad = dict(act=R.ACT_RELU_GRAD, residual=True, preact=True)
    return (_both(base)
            + _both(replace(base, name="batch3-broadcastA", a_broadcast=True, b_layout=MN_, seed=301))
            + _both(replace(base, name="batch3-aux-res-pre", seed=302, **grad))
            + _both(replace(base, name="batch3-split3", split_k=3, a_layout=MN_, bias_mode=R.BIAS_ROW, seed=303,
                            **grad))
            + _both(replace(base, name="batch3-broadcastA-split3", a_broadcast=True, split_k=3, seed=304, **grad))
            + _both(Case(name="batch_inner", M=70, N=36, K=40, batch=6, batch_inner=3, alpha=-2.0, beta=0.25,
                         bias_mode=R.BIAS_COL, act=R.ACT_RELU, b_layout=MN_, seed=305)))


def _geometries(c):
    n, h, w = 2, 5, 7
    out = []
    for mode in (R.PAD_ZERO, R.PAD_REPLICATE):
        out += [("3x3p1", Conv(n, h, w, c, 5, 7, 3, 3, 1, 1, mode)),
                ("1x3", Conv(n, h, w, c, 5, 5, 1, 3, 1, 0, mode)),
                ("1x1crop", Conv(n, h, w, c, 3, 5, 1, 1, 1, -1, mode)),
                ("1x1p1", Conv(n, h, w, c, 7, 9, 1, 1, 1, 1, mode)),
                ("4x4s2same", Conv(n, h, w, c, 3, 4, 4, 4, 2, 1, mode))]
    return [(f"{name}-{'zero' if cv.pad_mode == R.PAD_ZERO else 'replicate'}-c{c}", cv) for name, cv in out]


def conv_cases():
    """Implicit-im2col operands, exact regime: as A (forward / data gradient) with a row or a
    column bias, one gradient activation and split_k 1 / 3; as B (weight gradient) with rowsum_a."""
    out = []
    i = 0
    for c in (4, 12):
        for name, cv in _geometries(c):
            pixels, taps = cv.n * cv.oh * cv.ow, cv.kh * cv.kw * cv.c
            split = (1, 3)[i % 2]
            ep = (dict(bias_mode=R.BIAS_COL, act=R.ACT_RELU_GRAD, alpha=0.5, preact=True),
                  dict(bias_mode=R.BIAS_ROW, act=R.ACT_RELU, alpha=-2.0, beta=0.25, residual=True),
                  dict(bias_mode=R.BIAS_COL, act=R.ACT_LEAKY, row_scale_group=pixels // 2))[i % 3]
            out += _both(Case(name="convA-" + name, M=pixels, N=10, K=taps, a_layout=CV_, b_layout=(K_, MN_)[i % 2],
                              conv=cv, split_k=split, seed=400 + i, **ep))
            out += _both(Case(name="convB-" + name, M=10, N=taps, K=pixels, a_layout=MN_, b_layout=CV_, conv=cv,
                              split_k=split, rowsum=True, alpha=(1.0, 0.5)[i % 2], seed=450 + i))
            i += 1
    return out


def smooth_epilogue_cases():
    """Smooth activations on an exact pre-activation: integer operands and a power-of-two alpha
    put alpha * acc + bias in about [-8, 8]; the only error is the activation's own."""
    out = []
    acts = (R.ACT_GELU, R.ACT_SILU, R.ACT_SIGMOID, R.ACT_GELU_GRAD, R.ACT_SILU_GRAD)
    for i, act in enumerate(acts):
        pair = list(LAYOUT_PAIRS)[i % 4]
        al, bl = LAYOUT_PAIRS[pair]
        out += _both(Case(name=f"smooth-act{act}-{pair}", M=257, N=193, K=70, a_layout=al, b_layout=bl, alpha=2.0 ** -4,
                          bias_mode=(R.BIAS_COL, R.BIAS_ROW)[i % 2], act=act, preact=True, residual=i % 2 == 0,
                          split_k=(1, 2)[i % 2], regime="smooth", seed=500 + i))
        out += _both(Case(name=f"smooth-act{act}-batch3", M=70, N=36, K=70, batch=3, a_layout=al, b_layout=bl,
                          alpha=2.0 ** -4, bias_mode=R.BIAS_COL, act=act, preact=True, residual=True,
                          regime="smooth", seed=520 + i))
    return out


def gelu_load_cases():
    """MDEMI_OP_GELU on load (a k-contiguous A, or an n-contiguous B), K <= 128, plain epilogue."""
    out = []
    for i, (M, N, K) in enumerate(((129, 130, 70), (64, 64, 33), (130, 68, 128))):
        for bl in (K_, MN_):
            out += _both(Case(name=f"geluA-{M}x{N}x{K}-b{bl}", M=M, N=N, K=K, a_layout=K_, b_layout=bl, a_op=R.OP_GELU,
                              regime="smooth", seed=600 + 2 * i + bl))
        for al in (K_, MN_):
            out += _both(Case(name=f"geluB-{M}x{N}x{K}-a{al}", M=M, N=N, K=K, a_layout=al, b_layout=MN_, b_op=R.OP_GELU,
                              regime="smooth", seed=620 + 2 * i + al))
    return out


def exact_cases():
    return ([c for s in SHAPES for p in LAYOUT_PAIRS for c in shape_cases(s, p)] + combine_cases() + deep_cases()
            + batch_cases() + conv_cases())


def smooth_bound(d, ref):
    """Per-element tolerance of the smooth regime, float64: the suite's standing fp32 standard
    2e-5 * (1 + |ref|) for an epilogue activation on an exact pre-activation; for GELU on load
    2e-5 * (1 + sum_k |gelu(a)| |b|) (the rounding term K * 2^-24 stays below it for K <= 128)."""
    if d.a_op == R.OP_GELU or d.b_op == R.OP_GELU:
        assert d.K <= 128
        mag = torch.bmm(R.operand(d, "A").abs().contiguous(), R.operand(d, "B").abs().contiguous())
        return 2e-5 * (1.0 + mag)
    return 2e-5 * (1.0 + ref.abs())
