"""The GEMM descriptor contract (mdemi_gemm_desc, include/mdemi.h) against the fp64 reference
of tests/gemm_contract_ref.py, element by element.

Exact regime (tests/gemm_contract_cases.py): integer data on which every partial sum and every
epilogue stage is an fp32 number, so C, preact and rowsum_a must equal the fp64 reference
rounded to fp32 bit for bit (torch.equal) -- for every variant, raster, K split and combine
path of mdemi_gemm_f32, and, the operands being bf16 numbers, of mdemi_gemm_f32e and
mdemi_gemm_bf16 too.  Smooth regime: the activations and GELU on load, per element within
2e-5 * (1 + |ref|) resp. 2e-5 * (1 + sum_k |gelu(a)| |b|) (gemm_contract_cases.smooth_bound);
neither tolerance was measured on the code under test.

Every launch works on views into larger allocations the test owns: NaN around the inputs, a
NaN bit pattern around the outputs and in C itself when beta == 0.  After the call the outputs
equal the reference, none is NaN, and every slack word still holds its pattern."""
import functools

import pytest
import torch

import gemm_contract_cases as G
import gemm_contract_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_VARIANTS = (0, 1, 6, 8, 10, 12)  # one per LDS image kind, each tile height, the DMA variants, the 192-column tile
M16_VARIANTS = (0, 1, 2, 3, 4)
FAMILIES = ("fp32", "fp32e", "bf16")


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


class forced:
    """Forced variant / raster / combine settings, restored to the defaults on exit."""

    def __init__(self, variant=-1, group_m=8, m16=-1, inline=0):
        from mdemi import _lib as L
        self.L, self.lib, self.args = L, L.load(), (variant, group_m, m16, inline)

    def __enter__(self):
        variant, group_m, m16, inline = self.args
        self.L.check(self.lib.mdemi_gemm_set_variant(variant, group_m), "set_variant")
        self.L.check(self.lib.mdemi_gemm_set_variant_m16(m16), "set_variant_m16")
        self.L.check(self.lib.mdemi_gemm_set_options(1, inline), "set_options")
        return self

    def __exit__(self, *exc):
        self.lib.mdemi_gemm_set_variant(-1, 8)
        self.lib.mdemi_gemm_set_variant_m16(-1)
        self.lib.mdemi_gemm_set_options(1, 0)  # the defaults: tail split on, separate split-K reduce
        return False


class family:
    """mf.gemm on the fp32-operand entry point of one family (bf16 storage off: the bf16-operand
    path has its own tests), restored on exit."""

    def __init__(self, mf, name):
        self.mf, self.name = mf, name

    def __enter__(self):
        self.prev = (self.mf.get_matmul_precision(), self.mf.get_bf16_storage())
        self.mf.set_matmul_precision(self.name)
        self.mf.set_bf16_storage(False)

    def __exit__(self, *exc):
        self.mf.set_matmul_precision(self.prev[0])
        self.mf.set_bf16_storage(self.prev[1])
        return False


INPUTS = ("A", "B", "bias", "aux", "residual", "row_scale")


@functools.lru_cache(maxsize=4)
def prepared(case):
    """The case's descriptor, its reference (computed once, on the CPU in fp64) and pristine
    device copies of every allocation."""
    d = G.build(case)
    exact = case.regime == "exact"
    ref = R.expected(d, round32=exact)
    if exact:
        assert set(ref.inexact) <= ({"act", "row_scale"} if case.act == R.ACT_LEAKY else set()), (case.name, ref.inexact)
    p = dict(d=d, case=case, exact=exact)
    p["inputs"] = {n: getattr(d, n).to(DEV) for n in INPUTS if getattr(d, n) is not None}
    p["outputs"] = {n: getattr(d, n).to(DEV) for n in G.OUTPUTS if getattr(d, n) is not None}
    p["masks"] = {n: m.to(DEV) for n, m in d.masks.items()}
    want = {"C": ref.C, "preact": ref.preact, "rowsum_a": ref.rowsum_a}
    p["want64"] = {n: v.to(DEV) for n, v in want.items() if v is not None}
    p["want32"] = {n: v.float() for n, v in p["want64"].items()}
    p["bound"] = None if exact else G.smooth_bound(d, ref.C).to(DEV)
    return p


def launch(mf, p, outs, drop=()):
    from mdemi import _lib as L
    d, inp = p["d"], p["inputs"]

    def view(name):
        if name in drop:
            return None
        buf = outs.get(name, inp.get(name))
        return None if buf is None else buf[getattr(d, name + "_off", 0):]

    conv = None
    if d.conv is not None:
        c = d.conv
        conv = L.ConvGeom(n=c.n, h=c.h, w=c.w, c=c.c, oh=c.oh, ow=c.ow, kh=c.kh, kw=c.kw, stride=c.stride, pad=c.pad,
                          pad_mode=c.pad_mode)
    inner = (d.batch_inner, d.a_bstride_inner, d.b_bstride_inner, d.c_bstride_inner) if d.batch_inner > 1 else None
    mf.gemm(view("A"), view("B"), view("C"), d.M, d.N, d.K, lda=d.lda, ldb=d.ldb, ldc=d.ldc, a_layout=d.a_layout,
            b_layout=d.b_layout, a_op=d.a_op, b_op=d.b_op, alpha=d.alpha, beta=d.beta, bias=view("bias"),
            bias_mode=d.bias_mode, act=d.act, aux=view("aux"), ldaux=d.ldaux, residual=view("residual"),
            ldres=d.ldres, batch=d.batch, a_bstride=d.a_bstride, b_bstride=d.b_bstride, c_bstride=d.c_bstride,
            aux_bstride=d.aux_bstride, res_bstride=d.res_bstride, split_k=d.split_k, conv=conv,
            preact=view("preact"), ldpre=d.ldpre, pre_bstride=d.pre_bstride, rowsum_a=view("rowsum_a"), inner=inner,
            row_scale=view("row_scale"), row_scale_group=d.row_scale_group)


def run(mf, case, what):
    """One launch of `case` under the current settings on fresh copies of the output allocations,
    then: outputs equal the reference, no NaN, every slack word intact."""
    p = prepared(case)
    outs = {n: t.clone() for n, t in p["outputs"].items()}
    launch(mf, p, outs)
    what = f"{case.name} [{what}]"
    for name, buf in outs.items():
        got = G.logical(p["d"], name, buf)
        if p["exact"] or name == "preact":  # the pre-activation of the smooth epilogue cases is exact too
            G.check_exact(got, p["want32"][name], f"{what} {name}")
        else:
            G.check_close(got, p["want64"][name], p["bound"], f"{what} {name}")
        G.check_slack(buf, p["masks"][name], f"{what} {name}")


def sweep(mf, cases, f32=F32_VARIANTS, rasters=(0, 8), m16=M16_VARIANTS, inline=(0,), families=FAMILIES, default=True):
    for case in cases:
        for fam in families:
            with family(mf, fam):
                for il in inline:
                    if fam == "fp32":
                        settings = [(v, gm, -1) for v in f32 for gm in rasters] + ([(-1, 8, -1)] if default else [])
                    else:
                        settings = [(-1, 8, v) for v in m16] + [(-1, 0, m16[0])]
                    for v, gm, v16 in settings:
                        with forced(v, gm, v16, il):
                            run(mf, case, f"{fam} variant {v if fam == 'fp32' else v16} group_m {gm} inline {il}")


@pytest.mark.parametrize("pair", list(G.LAYOUT_PAIRS))
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_layouts_variants(mf, shape, pair):
    """Every tiling edge in all four dense layout pairs, aligned and misaligned, a full epilogue
    (alpha, beta, row or column bias, preact, activation, row_scale, residual; rowsum_a on an
    m-contiguous A): forced fp32 variants under both rasters, the autotuned default, and the
    16-bit families' variants -- all bit-equal to the fp64 reference."""
    sweep(mf, G.shape_cases(shape, pair))


@pytest.mark.parametrize("case", G.combine_cases(), ids=lambda c: c.name)
def test_combine_paths(mf, case):
    """Split-K (1, 3, 7 and more pieces than chunks) over a full epilogue: the separate reduce
    kernel (epilogue_value; N % 4 == 0 and != 0) and the inline combine apply the same stages."""
    sweep(mf, [case], f32=(0, 6, 10), rasters=(8,), m16=(0, 4), inline=(0, 1), default=False)


@pytest.mark.parametrize("case", G.deep_cases(), ids=lambda c: c.name)
def test_deep_split(mf, case):
    """split_k = 33 over 33 chunks: the column-sum combine where it may engage (ldc == N, plain
    store), and the ordinary combine with ldc > N, with a row_scale (which the column sums cannot
    apply) and with rowsum_a."""
    sweep(mf, [case], f32=(0, 10), rasters=(8,), m16=(0, 4), inline=(0, 1), default=False)


@pytest.mark.parametrize("case", G.batch_cases(), ids=lambda c: c.name)
def test_batched(mf, case):
    """batch 3 with per-batch aux / residual / preact strides, a broadcast A, split_k 3, and a
    two-level batch (heads as column slices) with an offset C."""
    sweep(mf, [case], f32=(0, 1, 6, 12), rasters=(0, 8), m16=(0, 2, 3))


@pytest.mark.parametrize("which", ["convA", "convB"])
@pytest.mark.parametrize("channels", [4, 12])
def test_conv_operands(mf, which, channels):
    """Implicit im2col as A and as B (weight gradient, with rowsum_a): 3x3 pad 1, 1x3, 1x1 crop
    (pad -1), 1x1 pad 1, 4x4 stride 2 with TF-'same' bottom/right padding; zero and replicate."""
    cases = [c for c in G.conv_cases() if c.name.startswith(which) and c.conv.c == channels]
    assert len(cases) == 20
    sweep(mf, cases, f32=(0, 1, 6, 8), rasters=(8,), m16=(0, 2, 3), default=False)


@pytest.mark.parametrize("case", G.smooth_epilogue_cases(), ids=lambda c: c.name)
def test_smooth_activations(mf, case):
    """GELU, SILU, SIGMOID, GELU_GRAD, SILU_GRAD on an exact pre-activation in about [-8, 8]
    (preact itself bit-equal), with batch 1 and with per-batch aux strides: per element within
    2e-5 * (1 + |ref|); in-kernel epilogue, reduce kernel and inline combine."""
    sweep(mf, [case], f32=(0, 6, 10), rasters=(8,), m16=(0,), inline=(0, 1), default=False)


@pytest.mark.parametrize("case", G.gelu_load_cases(), ids=lambda c: c.name)
def test_gelu_on_load(mf, case):
    """a_op / b_op = MDEMI_OP_GELU, K <= 128: per element within 2e-5 * (1 + sum_k |gelu(a)| |b|)."""
    sweep(mf, [case], f32=(0, 1, 6, 8), rasters=(8,), families=("fp32",))


REJECTED = {
    "rowsum_a with a k-contiguous A": (G.Case(name="rej-rowsum", M=40, N=24, K=36, rowsum=True), ()),
    "row_scale with batch 2": (G.Case(name="rej-row_scale", M=40, N=24, K=36, batch=2, row_scale_group=8), ()),
    "batch_inner with a residual": (G.Case(name="rej-inner", M=40, N=24, K=36, batch=4, batch_inner=2, residual=True), ()),
    "a gradient activation without aux": (G.Case(name="rej-aux", M=40, N=24, K=36, act=R.ACT_RELU_GRAD), ("aux",)),
    "a conv operand with c % 4 != 0": (G.Case(name="rej-conv", M=70, N=24, K=54, a_layout=R.L_CONV,
                                              conv=G.Conv(2, 5, 7, 6, 5, 7, 3, 3, 1, 1, R.PAD_ZERO)), ()),
}


@pytest.mark.parametrize("why", list(REJECTED))
def test_rejected_descriptors(mf, why):
    """Descriptors outside the contract are refused with MDEMI_EINVAL before any launch: C, filled
    with the pattern, is untouched."""
    case, drop = REJECTED[why]
    d = G.build(case)
    p = dict(d=d, inputs={n: getattr(d, n).to(DEV) for n in INPUTS if getattr(d, n) is not None})
    for fam in FAMILIES:
        with family(mf, fam):
            outs = {n: getattr(d, n).to(DEV) for n in G.OUTPUTS if getattr(d, n) is not None}
            with pytest.raises(RuntimeError, match=r"rc=-1\)"):
                launch(mf, p, outs, drop=drop)
            torch.cuda.synchronize()
            for name, buf in outs.items():
                G.check_slack(buf, torch.zeros_like(d.masks[name]), f"{why} [{fam}] {name}")
