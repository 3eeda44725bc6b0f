"""mdemi_gemm_f32_pair against two mdemi_gemm_f32 launches at the same forced variant: every
output allocation (C, preact, rowsum_a) equal bit for bit, slack included.

Every tensor lives inside a larger allocation (tests/gemm_contract_cases.py: NaN around the
inputs, a NaN bit pattern around the outputs and in the outputs themselves), so a read or a
write past an extent shows.  Each case runs at forced variants 8 and 11 and under the tuner's
default, in both member orders; at a forced pair variant an eligible pair must report the
one-launch arm (mdemi_gemm_pair_last_arm), an ineligible one the two-launch arm."""
import pytest
import torch

import gemm_contract_cases as G
from gemm_plan_util import tail_plan_m_split

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARM_OF = {11: 1, 8: 2}  # forced variant -> the one-launch arm
SETTINGS = (8, 11, -1)


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


class forced:
    """Forced fp32 variant and pairing switches for the block; the defaults after."""

    def __init__(self, variant=-1, enabled=1, arm=-1):
        from mdemi import _lib as L
        self.L, self.lib, self.args = L, L.load(), (variant, enabled, arm)

    def __enter__(self):
        variant, enabled, arm = self.args
        self.L.check(self.lib.mdemi_gemm_set_variant(variant, 8), "set_variant")
        self.L.check(self.lib.mdemi_gemm_pair_set_options(enabled, arm), "pair_set_options")
        return self

    def __exit__(self, *exc):
        self.lib.mdemi_gemm_set_variant(-1, 8)
        self.lib.mdemi_gemm_pair_set_options(1, -1)
        return False


def _ld(cols):
    return (cols + 3) // 4 * 4 + 4


class Bufs:
    """The allocations of one run: inputs placed in NaN slack, outputs in the pattern."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.outs = []  # (name, device allocation, mask of its logical elements)

    def rand(self, rows, cols):
        return torch.randn(rows, cols, generator=self.g)

    def inp(self, values):
        rows, cols = values.shape
        ld = _ld(cols)
        buf, _ = G._place(values[None], 8, ld, [0])
        return buf.to(DEV)[8:], ld

    def vec(self, values):
        buf, _ = G._vector(values, 4)
        return buf.to(DEV)[4:]

    def out(self, name, rows, cols):
        ld = _ld(cols)
        buf, mask = G._place(torch.zeros(1, rows, cols), 8, ld, [0], output=True, fill=False)
        buf = buf.to(DEV)
        self.outs.append((name, buf, mask))
        return buf[8:], ld

    def out_vec(self, name, n):
        buf, mask = G._vector(torch.zeros(n), 4, output=True, fill=False)
        buf = buf.to(DEV)
        self.outs.append((name, buf, mask))
        return buf[4:]


def dgrad(b, M, N, K, tag, *, gelu_grad=False, epilogue=False, m_live=None, a=None, lda=None, a_op=0):
    """<KCONTIG, MNCONTIG>: C[M,N] = A[M,K] . B[K,N]"""
    from mdemi import _lib as L
    if a is None:
        av = b.rand(M, K)
        if m_live is not None:  # the dead samples' rows of A are never read
            av[(m_live == 0).repeat_interleave(M // m_live.numel())] = float("nan")
        a, lda = b.inp(av)
    bm, ldb = b.inp(b.rand(K, N))
    c, ldc = b.out(tag + ".C", M, N)
    kw = dict(A=a, B=bm, C=c, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_layout=L.L_KCONTIG, b_layout=L.L_MNCONTIG,
              split_k=1, a_op=a_op)
    if gelu_grad:
        aux, ldaux = b.inp(b.rand(M, N))
        kw.update(act=L.ACT_GELU_GRAD, aux=aux, ldaux=ldaux)
    if epilogue:  # bias, row_scale and residual
        res, ldres = b.inp(b.rand(M, N))
        kw.update(bias=b.vec(b.rand(1, N)[0]), bias_mode=L.BIAS_COL, residual=res, ldres=ldres,
                  row_scale=b.vec(torch.tensor([0.0, 1.25, 2.0, 1.0, 0.5])), row_scale_group=(M + 4) // 5)
    if m_live is not None:
        kw.update(m_live=m_live.to(DEV))
    return kw


def wgrad(b, M, N, K, tag, *, split_k=1, rowsum=False, k_live=None):
    """<MNCONTIG, MNCONTIG>: C[M,N] = A[K,M]^T . B[K,N]"""
    from mdemi import _lib as L
    av, bv = b.rand(K, M), b.rand(K, N)
    if k_live is not None:  # the dead samples' k rows are never read
        dead = (k_live == 0).repeat_interleave(K // k_live.numel())
        av[dead] = float("nan")
        bv[dead] = float("nan")
    a, lda = b.inp(av)
    bm, ldb = b.inp(bv)
    c, ldc = b.out(tag + ".C", M, N)
    kw = dict(A=a, B=bm, C=c, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_layout=L.L_MNCONTIG, b_layout=L.L_MNCONTIG,
              split_k=split_k)
    if rowsum:
        kw.update(rowsum_a=b.out_vec(tag + ".rowsum_a", M))
    if k_live is not None:
        kw.update(k_live=k_live.to(DEV))
    return kw


def _seq(mf, kws):
    for kw in kws:
        mf.gemm(**kw)


def compare(mf, build, what, expect_pair=True, settings=SETTINGS, orders=(0, 1)):
    """build(Bufs) -> [kw0, kw1].  Pair entry against two launches, per setting and order."""
    from mdemi import _lib as L
    lib = L.load()
    for v in settings:
        for order in orders:
            with forced(v):
                ref, got = Bufs(7), Bufs(7)
                kr, kg = build(ref), build(got)
                if order:
                    kr, kg = kr[::-1], kg[::-1]
                _seq(mf, kr)
                mf.gemm_pair(*kg)
                arm = lib.mdemi_gemm_pair_last_arm()
                torch.cuda.synchronize()
            tag = f"{what} [variant {v}, order {order}, arm {arm}]"
            if v in ARM_OF:
                assert arm == (ARM_OF[v] if expect_pair else 0), f"{tag}: wrong arm"
            elif not expect_pair:
                assert arm == 0, f"{tag}: an ineligible pair ran as one launch"
            assert len(ref.outs) == len(got.outs)
            for (name, rb, mask), (_, gb, _) in zip(ref.outs, got.outs):
                assert torch.equal(rb.view(torch.int32), gb.view(torch.int32)), f"{tag} {name}: differs from two launches"
                G.check_slack(gb, mask, f"{tag} {name}")
                logical = gb.view(torch.int32)[mask.to(DEV)]
                assert (logical != G.PATTERN).all().item(), f"{tag} {name}: an element was never written"


def test_ragged_tiles_no_split(mf):
    compare(mf, lambda b: [dgrad(b, 200, 136, 72, "m0", gelu_grad=True), wgrad(b, 136, 72, 200, "m1", rowsum=True)],
            "ragged")


def test_split_member_through_reduce(mf):
    compare(mf, lambda b: [wgrad(b, 136, 264, 1000, "m0", split_k=3, rowsum=True),
                           dgrad(b, 1000, 136, 264, "m1", epilogue=True)], "split3")


def test_liveness_masks(mf):
    """4 samples of 96 rows, samples 1 and 3 dead and their operand rows NaN: m_live on the
    input-gradient member, k_live on the weight-gradient member."""
    live = torch.tensor([1.0 / 0.7, 0.0, 1.0 / 0.7, 0.0])
    compare(mf, lambda b: [dgrad(b, 384, 136, 72, "m0", m_live=live), wgrad(b, 72, 136, 384, "m1", k_live=live)],
            "masks")


def test_both_members_tail_split(mf):
    """Both members combine inline (tail split), on disjoint ranges of the per-device counters."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = ((3968, 3200, 128), (3200, 3968, 128))
    if not all(tail_plan_m_split(M, N, K, cus) > 0 for M, N, K in shapes):
        pytest.skip(f"the tail split does not engage for {shapes} on {cus} CUs")
    compare(mf, lambda b: [dgrad(b, *shapes[0], "m0"), wgrad(b, *shapes[1], "m1")], "tail-split")


def _conv_member(b):
    from mdemi import _lib as L
    n, h, w, c, N = 2, 5, 7, 4, 12
    x = torch.randn(n * h * w, c, generator=b.g)
    buf, _ = G._place(x[None], 8, c, [0])
    wt, ldb = b.inp(b.rand(N, 9 * c))
    out, ldc = b.out("conv.C", n * h * w, N)
    conv = L.ConvGeom(n=n, h=h, w=w, c=c, oh=h, ow=w, kh=3, kw=3, stride=1, pad=1, pad_mode=L.PAD_ZERO)
    return dict(A=buf.to(DEV)[8:], B=wt, C=out, M=n * h * w, N=N, K=9 * c, lda=0, ldb=ldb, ldc=ldc,
                a_layout=L.L_CONV, b_layout=L.L_KCONTIG, split_k=1, conv=conv)


def test_ineligible_pairs_fall_back(mf):
    from mdemi import _lib as L
    compare(mf, lambda b: [_conv_member(b), wgrad(b, 136, 72, 200, "m1", rowsum=True)], "conv member",
            expect_pair=False)
    compare(mf, lambda b: [dgrad(b, 200, 136, 72, "m0", a_op=L.OP_GELU), wgrad(b, 136, 72, 200, "m1")],
            "a_op GELU member", expect_pair=False)

    def dependent(b):  # member 1's A is member 0's C
        k0 = wgrad(b, 136, 72, 200, "m0")
        return [k0, dgrad(b, 136, 40, 72, "m1", a=k0["C"], lda=k0["ldc"])]

    compare(mf, dependent, "dependent pair", expect_pair=False, orders=(0,))
    # a forced one-launch arm does not override the dependence either
    lib = L.load()
    with forced(11, 1, 1):
        ref, got = Bufs(7), Bufs(7)
        _seq(mf, dependent(ref))
        mf.gemm_pair(*dependent(got))
        assert lib.mdemi_gemm_pair_last_arm() == 0
        for (name, rb, _), (_, gb, _) in zip(ref.outs, got.outs):
            assert torch.equal(rb.view(torch.int32), gb.view(torch.int32)), name


def test_pairing_off(mf):
    """The setter turns pairing off: the library entry called directly runs two launches and
    reports arm 0 even with a one-launch arm forced, and gemm_pair does not enter it at all; a
    forced arm 0 likewise, a forced arm 1 / 2 runs that arm.  Values equal two launches throughout."""
    from mdemi import _lib as L
    lib = L.load()
    build = lambda b: [dgrad(b, 200, 136, 72, "m0", gelu_grad=True), wgrad(b, 136, 72, 200, "m1", rowsum=True)]  # noqa: E731
    import ctypes

    def same(ref, got, what):
        for (name, rb, _), (_, gb, _) in zip(ref.outs, got.outs):
            assert torch.equal(rb.view(torch.int32), gb.view(torch.int32)), (what, name)

    for enabled, arm, want in ((0, -1, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 1), (1, 2, 2)):
        # the library entry itself (these members need no workspace): with pairing off it runs
        # two launches whatever arm is forced, and says so
        with forced(-1, enabled, arm):
            ref, got = Bufs(7), Bufs(7)
            _seq(mf, build(ref))
            kws = build(got)  # holds the operands until the launch is in the stream
            d0, d1 = (mf._gemm_desc(**kw) for kw in kws)
            assert lib.mdemi_gemm_pair_workspace_size(ctypes.byref(d0), ctypes.byref(d1)) == 0
            L.check(lib.mdemi_gemm_f32_pair(ctypes.byref(d0), ctypes.byref(d1), L.stream()), "gemm_f32_pair")
            assert lib.mdemi_gemm_pair_last_arm() == want, (enabled, arm)
            torch.cuda.synchronize()
        same(ref, got, ("entry", enabled, arm))
        # gemm_pair: with pairing off it makes the two gemm() calls and never enters the library's
        # paired entry; with it on, the entry and no gemm() call
        with forced(-1, enabled, arm):
            ref, got = Bufs(7), Bufs(7)
            _seq(mf, build(ref))
            calls, orig_entry = [], lib.mdemi_gemm_f32_pair

            def counted_entry(*a):
                calls.append("entry")
                return orig_entry(*a)

            lib.mdemi_gemm_f32_pair = counted_entry
            try:
                mf.gemm_pair(*build(got))
            finally:
                lib.mdemi_gemm_f32_pair = orig_entry
            assert calls == ([] if not enabled else ["entry"]), (enabled, arm, calls)
            if enabled:
                assert lib.mdemi_gemm_pair_last_arm() == want, (enabled, arm)
            torch.cuda.synchronize()
        same(ref, got, ("gemm_pair", enabled, arm))
    # a wrapped functional.gemm sees both GEMMs, in order, and the paired entry is not taken
    seen, orig = [], mf.gemm

    def spy(A, B, C, M, N, K, **kw):
        seen.append((M, N, K))
        return orig(A, B, C, M, N, K, **kw)

    mf.gemm = spy
    try:
        ref, got = Bufs(7), Bufs(7)
        _seq(mf, build(ref))
        del seen[:]
        mf.gemm_pair(*build(got))
    finally:
        mf.gemm = orig
    assert seen == [(200, 136, 72), (136, 72, 200)]
    same(ref, got, "wrapped gemm")
