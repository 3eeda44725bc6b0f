"""DropPath skip at the kernel level: the liveness masks of mdemi_gemm_desc (m_live, k_live) and
mdemi_winattn_desc (sample_live).

Every comparison is exact (torch.equal semantics: equal as numbers, -0 == +0) and is made
against the same entry point called without a mask -- the path the reference tests pin.  A
dead row of C may hold one of two values (include/mdemi.h): the unmasked one, or what the
epilogue makes of a zero accumulator, which is the same call with A zeroed.  That skipping
really happens is shown by poisoning the skipped operand data with NaN."""
import pytest
import torch

from gemm_plan_util import tail_plan_m_split

pytestmark = pytest.mark.gpu
DEV = "cuda"
NVARIANTS = 13  # F32_VARIANTS (csrc/gemm_plan.h); test_gemm_plan.py holds the hook's bound to the table
VARIANTS = list(range(NVARIANTS)) + [-1]  # every forced variant, then the autotuned path
MASKS = ([1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1], [0, 1, 1, 0])
KEEP = 1.0 / 0.7  # a live entry is the DropPath scale 1 / (1 - p), not 1


@pytest.fixture(scope="module")
def mf():
    from mdemi import functional as mf
    from mdemi import _lib
    _lib.load()
    return mf


def _rand(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g)


def _mask(bits):
    return torch.tensor([KEEP if b else 0.0 for b in bits], device=DEV)


def _rows(bits, group, live):
    """bool [len(bits) * group]: the rows of the live (or dead) groups."""
    m = torch.tensor([bool(b) == live for b in bits], device=DEV)
    return m.repeat_interleave(group)


class _Variant:
    """Force a variant of the fp32 family (and split-K options) for the block; defaults after."""

    def __init__(self, v, tail=1, inline=0):
        self.v, self.tail, self.inline = v, tail, inline

    def __enter__(self):
        from mdemi import _lib as L
        lib = L.load()
        L.check(lib.mdemi_gemm_set_variant(self.v, 8), "set_variant")
        L.check(lib.mdemi_gemm_set_options(self.tail, self.inline), "set_options")

    def __exit__(self, *a):
        from mdemi import _lib as L
        lib = L.load()
        lib.mdemi_gemm_set_variant(-1, 8)
        lib.mdemi_gemm_set_options(1, 0)  # the defaults: tail split on, separate split-K reduce
        return False


def _same_rows(c, ref):
    return (c == ref).all(dim=1)


# --------------------------------------------------------------------------
# M side
# --------------------------------------------------------------------------


def _m_side_call(mf, layout, epi, a, w, extra, M, N, K, m_live, group):
    """One GEMM C[M,N] = A[M,K] . W with the epilogue `epi`; returns its outputs (C first)."""
    from mdemi import _lib as L
    c = torch.empty(M, N, device=DEV)
    kw = dict(lda=K, ldc=N, a_layout=L.L_KCONTIG, split_k=1)
    if layout == "fwd":  # W stored [N][K]
        kw.update(ldb=K, b_layout=L.L_KCONTIG)
    else:  # dgrad: W stored [K][N]
        kw.update(ldb=N, b_layout=L.L_MNCONTIG)
    outs = [c]
    if epi == "bias":
        kw.update(bias=extra["bias"], bias_mode=L.BIAS_COL)
    elif epi == "gelu_preact":
        pre = torch.empty(M, N, device=DEV)
        outs.append(pre)
        kw.update(bias=extra["bias"], bias_mode=L.BIAS_COL, act=L.ACT_GELU, preact=pre, ldpre=N)
    elif epi == "scale_res":
        kw.update(bias=extra["bias"], bias_mode=L.BIAS_COL, residual=extra["res"], ldres=N,
                  row_scale=extra["scale"], row_scale_group=group)
    elif epi == "gelu_grad":
        kw.update(act=L.ACT_GELU_GRAD, aux=extra["aux"], ldaux=N)
    mf.gemm(a, w, c, M, N, K, m_live=m_live, **kw)
    return outs


@pytest.mark.parametrize("epi", ["bias", "gelu_preact", "scale_res", "gelu_grad"])
@pytest.mark.parametrize("layout", ["fwd", "dgrad"])
def test_gemm_m_live(mf, layout, epi):
    """M = 4 x 300 rows against 128- and 256-row tiles (tiles straddle samples), every variant:
    live rows equal the unmasked call; a dead row equals the unmasked row or the row of the
    same call with A zeroed; with row_scale == m_live and a residual it equals the residual."""
    G, M, N, K = 300, 1200, 192, 96
    a = _rand(M, K, seed=1)
    w = _rand(N, K, seed=2) if layout == "fwd" else _rand(K, N, seed=2)
    extra = {"bias": _rand(N, seed=3), "res": _rand(M, N, seed=4), "aux": _rand(M, N, seed=5)}
    zero_a = torch.zeros_like(a)
    for v in VARIANTS:
        with _Variant(v):
            for bits in MASKS:
                mask = _mask(bits)
                extra["scale"] = mask
                got = _m_side_call(mf, layout, epi, a, w, extra, M, N, K, mask, G)
                plain = _m_side_call(mf, layout, epi, a, w, extra, M, N, K, None, G)
                zeroed = _m_side_call(mf, layout, epi, zero_a, w, extra, M, N, K, None, G)
                live, dead = _rows(bits, G, True), _rows(bits, G, False)
                for o, p, z in zip(got, plain, zeroed):
                    assert torch.equal(o[live], p[live]), f"variant {v} mask {bits}: live rows differ"
                    either = _same_rows(o, p) | _same_rows(o, z)
                    assert bool(either[dead].all()), f"variant {v} mask {bits}: a dead row holds a third value"
                if epi == "scale_res":
                    assert torch.equal(got[0][dead], extra["res"][dead]), f"variant {v} mask {bits}: not the residual"


def test_gemm_m_live_ignored_by_the_bf16_family(mf):
    """bias + GELU + preact + c16: the bf16 copy of the output exists on the bf16-operand path
    only, whose family ignores the masks (include/mdemi.h) -- every output, c16 included, is
    the unmasked call's."""
    from mdemi import _lib as L
    G, M, N, K = 300, 1200, 192, 96
    a, w, bias = _rand(M, K, seed=1), _rand(N, K, seed=2), _rand(N, seed=3)

    def run(m_live):
        c, pre = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
        c16 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        with mf.matmul_precision("bf16"):
            mf.gemm(a, w, c, M, N, K, lda=K, ldb=K, ldc=N, a_layout=L.L_KCONTIG, b_layout=L.L_KCONTIG, split_k=1,
                    bias=bias, bias_mode=L.BIAS_COL, act=L.ACT_GELU, preact=pre, ldpre=N, c16=c16, m_live=m_live)
        return c, pre, c16

    plain = run(None)
    for bits in MASKS:
        for o, p in zip(run(_mask(bits)), plain):
            assert torch.equal(o, p), f"mask {bits}"


@pytest.mark.parametrize("layout", ["fwd", "dgrad"])
def test_gemm_m_live_skips_whole_dead_tiles(mf, layout):
    """M = 2048, groups of 512, mask [1,0,0,1]: rows 512..1535 are whole dead tiles at either
    tile height.  With those A rows NaN the dead output rows must still be finite (the K loop
    did not run) and the live rows unchanged, for every variant."""
    from mdemi import _lib as L
    G, M, N, K = 512, 2048, 192, 96
    bits = [1, 0, 0, 1]
    a = _rand(M, K, seed=6)
    w = _rand(N, K, seed=7) if layout == "fwd" else _rand(K, N, seed=7)
    bias = _rand(N, seed=8)
    live, dead = _rows(bits, G, True), _rows(bits, G, False)
    poisoned = a.clone()
    poisoned[dead] = float("nan")
    kw = dict(lda=K, ldc=N, a_layout=L.L_KCONTIG, split_k=1, bias=bias, bias_mode=L.BIAS_COL)
    kw.update(dict(ldb=K, b_layout=L.L_KCONTIG) if layout == "fwd" else dict(ldb=N, b_layout=L.L_MNCONTIG))
    mask = _mask(bits)
    for v in VARIANTS:
        with _Variant(v):
            plain = mf.gemm(a, w, torch.empty(M, N, device=DEV), M, N, K, **kw)
            got = mf.gemm(poisoned, w, torch.empty(M, N, device=DEV), M, N, K, m_live=mask, **kw)
        assert torch.equal(got[live], plain[live]), f"variant {v}: live rows differ"
        assert bool(torch.isfinite(got[dead]).all()), f"variant {v}: a dead tile read its A rows"
        assert torch.equal(got[dead], bias.expand(int(dead.sum()), N)), f"variant {v}: not the zero-accumulator value"


def _tail_shape(cus):
    """The smallest 8-sample M x 1536 x 128 GEMM (rows per sample a multiple of 8) whose tail
    plan engages on `cus` compute units with the split rows inside the last sample."""
    N, K = 1536, 128
    for g in range(8, 1 << 14, 8):
        m_split = tail_plan_m_split(8 * g, N, K, cus)
        if m_split >= 7 * g:
            return g, 8 * g, N, K, m_split
    raise AssertionError(f"no tail-split shape found for {cus} compute units")


def test_gemm_m_live_tail_split(mf):
    """Tail split on, last sample and one other dead: the split rows lie in the dead last
    sample, so their K pieces run over no K tile, still write their zero slabs and still hand
    off to the last arriver, which runs the epilogue.  Every variant."""
    from mdemi import _lib as L
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    G, M, N, K, m_split = _tail_shape(cus)
    assert 0 < m_split < M
    bits = [1, 1, 0, 1, 1, 1, 1, 0]
    a, w, bias, res = _rand(M, K, seed=9), _rand(N, K, seed=10), _rand(N, seed=11), _rand(M, N, seed=12)
    mask = _mask(bits)
    live, dead = _rows(bits, G, True), _rows(bits, G, False)
    poisoned = a.clone()
    poisoned[m_split:] = float("nan")  # the split rows: whole dead tiles
    kw = dict(lda=K, ldb=K, ldc=N, a_layout=L.L_KCONTIG, b_layout=L.L_KCONTIG, split_k=1, bias=bias,
              bias_mode=L.BIAS_COL, residual=res, ldres=N, row_scale=mask, row_scale_group=G)
    for v in VARIANTS:
        with _Variant(v, tail=1, inline=0):
            plain = mf.gemm(a, w, torch.empty(M, N, device=DEV), M, N, K, **kw)
            got = mf.gemm(poisoned, w, torch.empty(M, N, device=DEV), M, N, K, m_live=mask, **kw)
        assert torch.equal(got[live], plain[live]), f"variant {v}: live rows differ"
        assert torch.equal(got[dead], res[dead]), f"variant {v}: dead rows are not the residual"


# --------------------------------------------------------------------------
# K side
# --------------------------------------------------------------------------


def _dead_chunk_rows(bits, group, K):
    """bool [K]: the k of the 32-element chunks (aligned from 0) in which every k is dead."""
    dead = _rows(bits, group, False)
    out = torch.zeros(K, dtype=torch.bool, device=DEV)
    for k0 in range(0, K, 32):
        if bool(dead[k0:k0 + 32].all()):
            out[k0:k0 + 32] = True
    return out


@pytest.mark.parametrize("split", [1, 3, 40])
def test_gemm_k_live_wgrad(mf, split):
    """dW[192,96] = dY^T X with the bias-gradient row sums over K = 4 x 300 rows, dY zero on
    the dead samples: C and the row sums equal the unmasked call for every variant, split 1, 3
    and 40 (the deep-split combine), inline reduce on and off -- and still do, finite, when X
    is NaN in the chunks that lie wholly in dead rows (they are never loaded)."""
    from mdemi import _lib as L
    G, M, N, K = 300, 192, 96, 1200
    dy_full, x = _rand(K, M, seed=13), _rand(K, N, seed=14)
    kw = dict(lda=M, ldb=N, ldc=N, a_layout=L.L_MNCONTIG, b_layout=L.L_MNCONTIG, split_k=split)

    def run(dy, xx, k_live):
        c, rs = torch.empty(M, N, device=DEV), torch.empty(M, device=DEV)
        mf.gemm(dy, xx, c, M, N, K, rowsum_a=rs, k_live=k_live, **kw)
        return c, rs

    for bits in MASKS:
        dy = dy_full.clone()
        dy[_rows(bits, G, False)] = 0.0
        poisoned = x.clone()
        poisoned[_dead_chunk_rows(bits, G, K)] = float("nan")
        mask = _mask(bits)
        for v in VARIANTS:
            for inline in (0, 1):
                with _Variant(v, tail=1, inline=inline):
                    c0, rs0 = run(dy, x, None)
                    c1, rs1 = run(dy, x, mask)
                    c2, rs2 = run(dy, poisoned, mask)
                tag = f"variant {v} split {split} inline {inline} mask {bits}"
                assert torch.equal(c1, c0) and torch.equal(rs1, rs0), tag
                assert bool(torch.isfinite(c2).all()), tag + ": a dead chunk was loaded"
                assert torch.equal(c2, c0) and torch.equal(rs2, rs0), tag + " (poisoned)"


# --------------------------------------------------------------------------
# window attention
# --------------------------------------------------------------------------


def _winattn(mf, qkv, bias, rpb, geo, dout, live):
    B, H, W, heads, C, shift = geo
    q, b, t = (x.detach().clone().requires_grad_() for x in (qkv, bias, rpb))
    out = mf.window_attention(q, b, q, b, t, B, H, W, heads, 7, shift, (C // heads) ** -0.5, C, v_off=2 * C,
                              live=live)
    lse = out.grad_fn.saved_tensors[6]
    out.backward(dout)
    return {"out": out.detach(), "lse": lse.view(B, -1), "dqkv": q.grad, "dbias": b.grad, "d_rpb": t.grad}


@pytest.mark.parametrize("shift", [0, 3])
def test_winattn_sample_live(mf, shift):
    """B = 3, 10 x 12 tokens (pads to 14 x 14), 2 heads of 32: live samples' out, lse, dq, dk, dv
    equal the unmasked call; dead samples' are zero; d_rpb and the pad sums (the qkv-bias
    gradient) equal the unmasked call run with the dead samples' dout zeroed."""
    B, H, W, heads, C = 3, 10, 12, 2, 64
    n = H * W
    qkv, bias = _rand(B * n, 3 * C, seed=15), _rand(3 * C, seed=16)
    rpb, dout = _rand(169, heads, seed=17) * 0.5, _rand(B * n, C, seed=18)
    geo = (B, H, W, heads, C, shift)
    plain = _winattn(mf, qkv, bias, rpb, geo, dout, None)
    for bits in ([1, 0, 1], [0, 0, 0]):
        got = _winattn(mf, qkv, bias, rpb, geo, dout, _mask(bits))
        dout0 = dout.clone()
        dout0[_rows(bits, n, False)] = 0.0
        plain0 = _winattn(mf, qkv, bias, rpb, geo, dout0, None)
        for name in ("out", "dqkv"):
            g, p = got[name].view(B, n, -1), plain[name].view(B, n, -1)
            for s, b in enumerate(bits):
                if b:
                    assert torch.equal(g[s], p[s]), f"{name}: live sample {s} differs (mask {bits})"
                else:
                    assert not bool(g[s].any()), f"{name}: dead sample {s} is not zero (mask {bits})"
        for s, b in enumerate(bits):
            if b:
                assert torch.equal(got["lse"][s], plain["lse"][s]), f"lse: live sample {s} differs"
            else:
                assert not bool(got["lse"][s].any()), f"lse: dead sample {s} is not zero"
        assert torch.equal(got["d_rpb"], plain0["d_rpb"]), f"d_rpb (mask {bits})"
        assert torch.equal(got["dbias"], plain0["dbias"]), f"pad sums (mask {bits})"
        assert torch.equal(got["dqkv"], plain0["dqkv"]), f"dqkv against a zeroed dout (mask {bits})"
