"""The fp64 reference of the window-attention descriptor contract, checked on the CPU before
the GPU tests (tests/test_winattn_contract_gpu.py) rely on it:

* its two formulations -- the index maps of the header and the pad / roll / partition
  restatement of the reference -- agree to 1e-12 on every case, forward and every gradient;
* it agrees with oracle.newcrfs's window_partition / shift_mask / _rel_bias composed by hand;
* dq_pad is exactly zero and lse is +inf exactly at the pad queries;
* the tolerances of the GPU tests are 4 x the error of the reference's own fp32 restatement,
  none above 1e-4;
* that criterion rejects every planted error on a named case;
* the exact-gather cases make at least a third of the real queries, and one of every window,
  bit-exact."""
import pytest
import torch

import winattn_contract_cases as G
import winattn_contract_ref as R

from oracle import newcrfs as onc


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.data_key() not in seen:
            seen.add(c.data_key())
            out.append(c)
    return out


LIVE_CASES = _unique(G.geometry_cases() + G.layout_cases() + G.gather_cases())
ALL_CASES = _unique(G.all_cases())
GRADS = ("dq", "dk", "dv", "d_rpb_table", "dq_pad", "dk_pad", "dv_pad")


def _agree(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= tol * max(1.0, b.abs().max().item() if b.numel() else 0.0), f"{what}: max|diff| {err:.3e}"


@pytest.mark.parametrize("case", LIVE_CASES, ids=lambda c: c.name)
def test_two_formulations_agree(case):
    p, C = G.problem(case), case.C
    zeros = torch.zeros(C, dtype=torch.float64)
    qk = torch.cat([p.q, p.k], 1).requires_grad_()
    qkb = torch.cat([p.q_pad if p.q_pad is not None else zeros, p.k_pad if p.k_pad is not None else zeros])
    qkb.requires_grad_()
    v = p.v.clone().requires_grad_()
    vb = (p.v_pad if p.v_pad is not None else zeros).clone().requires_grad_()
    rpb = p.rpb.clone().requires_grad_()
    out = R._ref_window_attn(qk, qkb, v, vb, rpb, p.B, p.H, p.W, p.heads, R.WS, p.shift, p.scale, C, 0)
    out.backward(p.dout)
    ref = p.ref
    _agree(out.detach(), ref["out"], "out")
    other = dict(dq=qk.grad[:, :C], dk=qk.grad[:, C:], dv=v.grad, d_rpb_table=rpb.grad, dq_pad=qkb.grad[:C],
                 dk_pad=qkb.grad[C:], dv_pad=vb.grad)
    for name in GRADS:
        _agree(other[name], ref[name], name)


@pytest.mark.parametrize("H,W,shift", [(3, 20, 1), (13, 15, 3), (8, 6, 6)])
def test_against_oracle_composition(H, W, shift):
    """F.pad with the pad vector, roll, oracle window_partition, _rel_bias, shift_mask, softmax,
    window_reverse, roll back, crop: out and lse of the index-map function."""
    B, heads, ws = 2, 3, R.WS
    case = G.Case(name="oracle", H=H, W=W, shift=shift, B=B, heads=heads, seed=900 + shift)
    p, C = G.problem(case), case.C
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws

    def windows(t, pad):
        full = pad.view(1, 1, 1, C).expand(B, Hp, Wp, C).clone()
        full[:, :H, :W] = t.view(B, H, W, C)
        full = torch.roll(full, (-shift, -shift), (1, 2))
        return onc.window_partition(full, ws).view(-1, ws * ws, heads, R.HD).transpose(1, 2)

    qw, kw, vw = windows(p.q, p.q_pad), windows(p.k, p.k_pad), windows(p.v, p.v_pad)
    attn = (qw * p.scale) @ kw.transpose(-2, -1) + onc._rel_bias(p.rpb, ws, heads).unsqueeze(0)
    mask = onc.shift_mask(H, W, ws, shift).double()
    nW = mask.shape[0]
    attn = (attn.view(B, nW, heads, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, ws * ws, ws * ws)
    o = (attn.softmax(-1) @ vw).transpose(1, 2).reshape(-1, ws, ws, C)
    o = torch.roll(onc.window_reverse(o, ws, Hp, Wp), (shift, shift), (1, 2))[:, :H, :W].reshape(-1, C)
    _agree(o, p.ref["out"], "out")
    lse = torch.logsumexp(attn, -1)
    real = p.ref["geom"].row >= 0
    got = p.ref["lse"]
    sel = real[:, None, :].expand_as(got)
    _agree(got[sel], lse[sel], "lse")


@pytest.mark.parametrize("case", LIVE_CASES, ids=lambda c: c.name)
def test_pad_queries(case):
    ref = G.problem(case).ref
    assert torch.equal(ref["dq_pad"], torch.zeros_like(ref["dq_pad"]))
    pad = (ref["geom"].row < 0)[:, None, :].expand_as(ref["lse"])
    assert torch.equal(torch.isposinf(ref["lse"]), pad)
    assert torch.isfinite(ref["lse"][~pad]).all().item()


@pytest.fixture(scope="module")
def fp32_errors():
    """Per output, the largest normalised error of the fp32 restatement over every case, and the
    case it occurs on."""
    worst = {}
    for case in ALL_CASES:
        p = G.problem(case)
        res = G.reference(p, torch.float32)
        for name in (("out", "lse") if case.gather else G.TOL):  # the gather cases are forward-only
            e = G.normalised_error(name, res[name], p.ref)
            if e > worst.get(name, (-1.0, None))[0]:
                worst[name] = (e, case.name)
    return worst


def test_tolerances_come_from_the_fp32_restatement(fp32_errors):
    for name, (e, where) in fp32_errors.items():
        print(f"{name:12s} fp32 restatement max {e:.3e} on {where}; TOL {G.TOL[name]:.3e}")
    assert fp32_errors["dq_pad"][0] == 0.0 and G.TOL["dq_pad"] == 0.0
    for name, (e, where) in fp32_errors.items():
        if name == "dq_pad":
            continue
        assert G.TOL[name] <= 1e-4, name
        assert G.TOL[name] >= 4 * G.MEASURED_FP32[name] and G.TOL[name] <= 4.4 * G.MEASURED_FP32[name], name
        assert 2 * e <= G.TOL[name] <= 8 * e, f"{name}: TOL {G.TOL[name]:.3e} is not 4 x {e:.3e} within a factor 2"


# planted error -> the case that must reject it, and an output on which it does
PLANTED = {
    "rpb_swapped": ("7x7s0-B1h1", "out"),
    "no_mask": ("7x7s3-B3h1", "out"),
    "region_boundary": ("13x15s3-B2h2", "out"),
    "pad_reads_zero": ("3x20s1-B2h3", "out"),
    "dq_unscaled": ("7x7s0-B1h1", "dq"),
    "dk_pad_dropped": ("10x12s3-B1h5", "dk_pad"),
    "head_shifted": ("7x7s0-B2h3", "out"),
    "roll_reversed": ("9x16s2-B2h3", "out"),
}


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_criterion_rejects_planted_error(flaw):
    where, name = PLANTED[flaw]
    case = next(c for c in G.geometry_cases() if c.name == where)
    p = G.problem(case)
    clean = G.reference(p, torch.float32)
    for n in G.TOL:
        G.check(n, clean[n], p.ref, f"{where} fp32 restatement")
    bad = G.reference(p, torch.float32, flaws=(flaw,))
    rejected = [n for n in G.TOL if not G.passes(n, bad[n], p.ref)]
    print(f"{flaw}: rejected on {where} by {rejected}")
    assert name in rejected, f"{flaw} passes the criterion on {name} of {where} (rejected: {rejected})"


@pytest.mark.parametrize("case", G.gather_cases(), ids=lambda c: c.name)
def test_gather_share(case):
    exact, want, per_window = G.gather_expected(case)
    share = exact.float().mean().item()
    print(f"{case.name}: {int(exact.sum())} of {exact.numel()} real queries exact, windows {per_window}")
    assert share >= 1 / 3, share
    assert all(per_window), per_window
    # the reference itself gathers: its out rows equal the picked rows to fp64 rounding
    ref = G.problem(case).ref["out"]
    assert torch.equal(ref[exact].float(), want[exact])
    assert {o for _, o in G.GATHER} == {(0, 1), (1, 0), (-1, -1)}
