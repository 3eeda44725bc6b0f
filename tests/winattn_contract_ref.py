"""mdemi_winattn_desc (include/mdemi.h) restated in plain torch on the CPU, twice.

attention(...) is the index-map formulation the header describes: window token (ty, tx) of
window (b, wy, wx) sits at rolled-padded (py, px) = (wy*7 + ty, wx*7 + tx) and gathers from
original padded ((py + s) % Hp, (px + s) % Wp); it is a pad token when that lies outside the
H x W grid; the shift mask compares the region ids of rolled-padded coordinates.  It takes what
the descriptor takes -- q, k, v as (storage, leading dimension, column offset), each pad vector
optional on its own -- and returns out, lse and, through autograd on fp64 leaves, every
gradient of the backward, with the absolute sums that scale the summed outputs (d_rpb_table and
the pad sums) in the comparison criterion.

_ref_window_attn(...) is the pad / roll / window_partition restatement of the reference's
SwinTransformerBlock + WindowAttention (swin_transformer.py:112-240), the formulation
tests/test_kernels_gpu.py::test_window_attention has always used.  The two share no code, so
their agreement (tests/test_winattn_contract_ref.py) checks both.

attention(dtype=torch.float32) runs the same function in fp32 throughout: it sizes the
tolerances of the GPU tests (winattn_contract_cases.TOL), nothing else.  `flaws` plants one
named error into it for the discrimination test."""
from collections import namedtuple
from types import SimpleNamespace

import torch

WS, HD, N, T = 7, 32, 49, 169

Operand = namedtuple("Operand", "data ld col")  # 1-D storage, leading dimension, first column

FLAWS = ("rpb_swapped", "no_mask", "region_boundary", "pad_reads_zero", "dq_unscaled", "dk_pad_dropped",
         "head_shifted", "roll_reversed")


def rows_of(op, rows, cols):
    """The [rows, cols] matrix an Operand describes."""
    return torch.as_strided(op.data, (rows, cols), (op.ld, 1), op.col)


def geometry(B, H, W, shift, flaws=()):
    """Index maps of the descriptor's geometry: row [nwin, 49] (the token-major row a window
    token reads, -1 for a pad token) and region [nwin, 49] (shift-mask region id), windows
    ordered (b, wy, wx)."""
    Hp, Wp = (H + WS - 1) // WS * WS, (W + WS - 1) // WS * WS
    nWh, nWw = Hp // WS, Wp // WS
    win = torch.arange(B * nWh * nWw)
    b, wy, wx = win // (nWh * nWw), win // nWw % nWh, win % nWw
    t = torch.arange(N)
    py = wy[:, None] * WS + t[None, :] // WS
    px = wx[:, None] * WS + t[None, :] % WS
    s = -shift if "roll_reversed" in flaws else shift
    oy, ox = (py + s) % Hp, (px + s) % Wp
    row = torch.where((oy < H) & (ox < W), (b[:, None] * H + oy) * W + ox, torch.full_like(oy, -1))
    edge = shift - 1 if "region_boundary" in flaws else shift

    def reg(p, full):
        return (p >= full - WS).long() + (p >= full - edge).long()

    region = reg(py, Hp) * 3 + reg(px, Wp)
    return SimpleNamespace(Hp=Hp, Wp=Wp, nwin=B * nWh * nWw, nwin_per_sample=nWh * nWw, row=row, region=region)


def rpb_slot():
    """slot[q, key] of the [169][heads] table: (qy - ky + 6) * 13 + (qx - kx + 6)."""
    t = torch.arange(N)
    y, x = t // WS, t % WS
    return (y[:, None] - y[None, :] + WS - 1) * (2 * WS - 1) + (x[:, None] - x[None, :] + WS - 1)


def attention(q, k, v, q_pad, k_pad, v_pad, rpb_table, B, H, W, heads, window=WS, shift=0, scale=1.0,
              dtype=torch.float64, flaws=()):
    """q, k, v: Operand; *_pad: [heads * 32] or None; rpb_table [169, heads].
    Returns r with r.out [rows, C], r.lse [nwin, heads, 49] (+inf at pad queries), r.geom, and
    r.backward(dout) -> dict of dq, dk, dv [rows, C], d_rpb_table [169, heads], dq_pad, dk_pad,
    dv_pad [C] (the gradients of the pad vectors as leaves, zeros standing in for a null one),
    and the criterion's scales: d_rpb_table_scale, dk_pad_scale, dv_pad_scale = the sum of the
    absolute values of the terms added into each element (score gradients per table slot, pad
    tokens' k / v gradient rows); dq_scale, dk_scale [rows, C] = the same for dq and dk, taken
    down to the products of inputs, because a score gradient P (dP - D) can cancel to zero."""
    assert window == WS and set(flaws) <= set(FLAWS)
    C, rows = heads * HD, B * H * W
    g = geometry(B, H, W, shift, flaws)
    real = g.row >= 0                      # [nwin, 49]
    src = g.row.clamp(min=0)

    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_()

    mats = [leaf(rows_of(op, rows, C)) for op in (q, k, v)]
    pads = [leaf(p if p is not None else torch.zeros(C)) for p in (q_pad, k_pad, v_pad)]
    table = leaf(rpb_table)
    if "head_shifted" in flaws:            # the last head reads v four columns to the right (wrapping in the head)
        vm = mats[2].view(rows, heads, HD)
        mats_v = torch.cat([vm[:, :-1], torch.roll(vm[:, -1:], -4, dims=2)], 1).reshape(rows, C)
    else:
        mats_v = mats[2]
    wins = []
    for i, (m, p) in enumerate(zip((mats[0], mats[1], mats_v), pads)):
        padv = p
        if "pad_reads_zero" in flaws:
            padv = torch.zeros_like(p)
        if "dk_pad_dropped" in flaws and i == 1:
            padv = p.detach()
        w_ = torch.where(real[:, :, None], m[src], padv.view(1, 1, C).expand(g.nwin, N, C))
        w_.retain_grad()
        wins.append(w_)
    qw, kw, vw = wins

    def split(w_):                         # [nwin, 49, C] -> [nwin, heads, 49, 32]
        return w_.view(g.nwin, N, heads, HD).transpose(1, 2)

    qs = split(qw) * scale
    if "dq_unscaled" in flaws:             # same value, gradient without the factor
        qs = split(qw.detach()) * scale + (split(qw) - split(qw.detach()))
    slot = rpb_slot()
    if "rpb_swapped" in flaws:
        slot = slot.t()
    bias = table[slot.reshape(-1)].view(N, N, heads).permute(2, 0, 1)      # [heads, q, key]
    S = qs @ split(kw).transpose(-2, -1) + bias.unsqueeze(0)
    if shift > 0 and "no_mask" not in flaws:
        differ = g.region[:, :, None] != g.region[:, None, :]               # [nwin, q, key]
        S = S + torch.where(differ, -100.0, 0.0).to(dtype).unsqueeze(1)
    S.retain_grad()
    lse = torch.logsumexp(S, -1)                                            # [nwin, heads, 49]
    P = torch.exp(S - lse.unsqueeze(-1))
    ow = (P @ split(vw)).transpose(1, 2).reshape(g.nwin, N, C)
    out = torch.zeros(rows, C, dtype=dtype).index_copy(0, g.row[real], ow[real])
    r = SimpleNamespace(geom=g, out=out.detach(), P=P.detach(),
                        lse=torch.where(real[:, None, :], lse.detach(), torch.full_like(lse.detach(), float("inf"))))

    def backward(dout):
        out.backward(rows_of(dout, rows, C).to(dtype) if isinstance(dout, Operand) else dout.to(dtype))
        pad_tok = (~real)[:, :, None].to(dtype)
        slot_abs = torch.zeros(T, heads, dtype=dtype).index_add_(
            0, slot.reshape(-1), S.grad.abs().sum(0).permute(1, 2, 0).reshape(N * N, heads))

        def grad(t):  # a leaf nothing depends on (no pad token; a planted error) has a zero gradient
            return t.grad if t.grad is not None else torch.zeros_like(t)

        # dq / dk are sums of dS K / dS^T Q with dS = P (dP - D), dP = V dO^T, D = rowsum(dO o O): the
        # absolute values of everything added into an element, taken down to the products of inputs
        with torch.no_grad():
            dow = torch.zeros(g.nwin, N, C, dtype=dtype)
            dow[real] = (rows_of(dout, rows, C) if isinstance(dout, Operand) else dout).to(dtype)[g.row[real]]
            dp_abs = split(dow).abs() @ split(vw).abs().transpose(-2, -1)              # [nwin, heads, q, key]
            d_abs = (split(dow).abs() * split(ow).abs()).sum(-1, keepdim=True)         # [nwin, heads, q, 1]
            w_abs = P * (dp_abs + d_abs)

            def to_rows(t):                                                            # [nwin, heads, tok, 32]
                t = t.transpose(1, 2).reshape(g.nwin, N, C)
                return torch.zeros(rows, C, dtype=dtype).index_copy(0, g.row[real], t[real])

            dq_abs = to_rows(scale * (w_abs @ split(kw).abs()))
            dk_abs = to_rows(scale * (w_abs.transpose(-2, -1) @ split(qw).abs()))
        return dict(dq=grad(mats[0]), dk=grad(mats[1]), dv=grad(mats[2]), d_rpb_table=grad(table),
                    dq_pad=grad(pads[0]), dk_pad=grad(pads[1]), dv_pad=grad(pads[2]),
                    d_rpb_table_scale=slot_abs, dq_scale=dq_abs, dk_scale=dk_abs,
                    dk_pad_scale=(kw.grad.abs() * pad_tok).sum((0, 1)),
                    dv_pad_scale=(vw.grad.abs() * pad_tok).sum((0, 1)))

    r.backward = backward
    return r


def _ref_window_attn(qk, qk_bias, v, v_bias, rpb, B, H, W, heads, ws, shift, scale, C, v_off):
    """Direct restatement of WindowAttention + pad/roll/partition (swin_transformer.py:112-240)."""
    hd = C // heads
    rows = B * H * W
    q = qk[:, :C]
    k = qk[:, C:2 * C]
    vv = v[:, v_off:v_off + C]
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws

    def grid(t, pad):
        t = t.view(B, H, W, C)
        full = (pad.view(1, 1, 1, C) if pad is not None else torch.zeros(1, 1, 1, C, dtype=t.dtype)).expand(
            B, Hp, Wp, C).clone()
        full[:, :H, :W] = t
        if shift:
            full = torch.roll(full, (-shift, -shift), (1, 2))
        return full.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)

    qw = grid(q, qk_bias[:C] if qk_bias is not None else None)
    kw = grid(k, qk_bias[C:2 * C] if qk_bias is not None else None)
    vw = grid(vv, v_bias[v_off:v_off + C] if v_bias is not None else None)
    nW = qw.shape[0] // B
    qh = qw.view(-1, ws * ws, heads, hd).transpose(1, 2) * scale
    kh = kw.view(-1, ws * ws, heads, hd).transpose(1, 2)
    vh = vw.view(-1, ws * ws, heads, hd).transpose(1, 2)
    attn = qh @ kh.transpose(-2, -1)
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0)
    idx = (rel[..., 0] + ws - 1) * (2 * ws - 1) + rel[..., 1] + ws - 1
    attn = attn + rpb[idx.view(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1).unsqueeze(0)
    if shift:
        img = torch.zeros(1, Hp, Wp, 1, dtype=qk.dtype)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 1
        mw = img.view(1, Hp // ws, ws, Wp // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)
        attn = attn.view(B, nW, heads, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, ws * ws, ws * ws)
    attn = attn.softmax(-1)
    o = (attn @ vh).transpose(1, 2).reshape(-1, ws * ws, C)
    o = o.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o[:, :H, :W].reshape(rows, C)
