"""The fp64 reference of the normalisation contract (tests/norm_contract_ref.py) and the cases
of tests/norm_contract_cases.py, checked on the CPU before the GPU tests rely on them:

* the restatement of the header's formulas agrees with torch's own layer_norm / batch_norm /
  group_norm and their autograd to 1e-12 in fp64, on every case and every activation;
* the tolerances are 4 x the error of the reference's fp32 restatement (sequential fp32 sums),
  none above what the existing kernel tests grant (1e-5 forward, 1e-4 gradients);
* every BatchNorm case has the launch-geometry property it is named for, and no element of a
  kinked case lies within the margin of the kink;
* the criterion rejects every planted error on a named case."""
import pytest
import torch
import torch.nn.functional as F

import norm_contract_cases as G
import norm_contract_ref as R

D = torch.float64


def _agree(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), f"{what}: max|diff| {err:.3e}"


def _torch_act(act, v):
    return {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_LEAKY: lambda t: F.leaky_relu(t, 0.01), R.ACT_SILU: F.silu,
            R.ACT_GELU: F.gelu}[act](v)


# ---------------------------------------------------------------------------------------------
# two formulations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.LN_CASES, ids=lambda c: c.name)
def test_layernorm_two_formulations(case):
    p = G.ln_problem(case)
    x, g, b = p.x.clone().requires_grad_(), p.gamma.clone().requires_grad_(), p.beta.clone().requires_grad_()
    y = F.layer_norm(x, (p.C,), g, b, p.eps)
    y.backward(p.dy)
    f = R.layernorm_fwd(p.x, p.gamma, p.beta, p.eps)
    bw = R.layernorm_bwd(p.dy, p.x, f["mean"], f["rstd"], p.gamma)
    _agree(f["y"], y.detach(), "y")
    _agree(f["mean"], p.x.mean(1), "mean")
    _agree(f["rstd"], 1 / torch.sqrt(p.x.var(1, unbiased=False) + p.eps), "rstd")
    _agree(bw["dx"], x.grad, "dx")
    _agree(bw["dgamma"], g.grad, "dgamma")
    _agree(bw["dbeta"], b.grad, "dbeta")
    added = R.layernorm_bwd(p.dy, p.x, f["mean"], f["rstd"], p.gamma, add=p.dadd)
    _agree(added["dx"], x.grad + p.dadd, "dx + dadd")


def _bn_two_formulations(p, act):
    rows, C = p.rows, p.C
    if rows == 1:  # torch refuses to train on one value per channel; the header's formulas do not
        f = R.bn_train_fwd(p.x, p.gamma, p.beta, p.running_mean0, p.running_var0, p.momentum, p.eps, act)
        bw = R.chnorm_bwd(p.dy, p.x, f["mean"], f["rstd"], p.gamma, p.beta, C, 1, act)
        assert torch.equal(f["mean"], p.x[0, 0]) and torch.equal(f["y"][0, 0], R.act_fwd(act, p.beta))
        assert torch.equal(f["running_var"], (1 - p.momentum) * p.running_var0)
        assert torch.equal(bw["dx"], torch.zeros_like(bw["dx"])) and torch.equal(bw["dgamma"], torch.zeros_like(p.gamma))
        assert torch.equal(bw["dbeta"], (p.dy * R.act_grad(act, p.beta))[0, 0])
        return
    x, g, b = (t.clone().requires_grad_() for t in (p.x.reshape(rows, C), p.gamma, p.beta))
    rm, rv = p.running_mean0.clone(), p.running_var0.clone()
    y = _torch_act(act, F.batch_norm(x, rm, rv, g, b, True, p.momentum, p.eps))
    y.backward(p.dy.reshape(rows, C))
    f = R.bn_train_fwd(p.x, p.gamma, p.beta, p.running_mean0, p.running_var0, p.momentum, p.eps, act)
    _agree(f["y"].reshape(rows, C), y.detach(), "y")
    _agree(f["mean"], p.x.reshape(rows, C).mean(0), "mean")
    _agree(f["running_mean"], rm, "running_mean")
    _agree(f["running_var"], rv, "running_var")
    _agree(f["pooled"], y.detach().view(p.N, p.HW, C).mean(1), "pooled")
    bw = R.chnorm_bwd(p.dy, p.x, f["mean"], f["rstd"], p.gamma, p.beta, C, 1, act)
    _agree(bw["dx"].reshape(rows, C), x.grad, "dx")
    _agree(bw["dgamma"], g.grad, "dgamma")
    _agree(bw["dbeta"], b.grad, "dbeta")
    ru = R.bn_running_update(f["mean"], f["rstd"], p.running_mean0, p.running_var0, rows, p.eps, p.momentum)
    _agree(ru["running_mean"], f["running_mean"], "bn_running_update mean")
    _agree(ru["running_var"], f["running_var"], "bn_running_update var", 1e-10)
    # frozen statistics: eval-mode batch_norm with (mean, var) = the given (mean, 1 / rstd^2 - eps)
    x2, g2, b2 = (t.detach().clone().requires_grad_() for t in (x, g, b))
    mean, rstd = p.mean32, p.rstd32
    y2 = _torch_act(act, F.batch_norm(x2, mean.clone(), 1 / (rstd * rstd) - p.eps, g2, b2, False, 0.0, p.eps))
    y2.backward(p.dy.reshape(rows, C))
    fr = R.bn_frozen_bwd(p.dy, p.x, mean, rstd, p.gamma, p.beta, act)
    _agree(R.chnorm_apply(p.x, p.gamma, p.beta, mean, rstd, C, 1, act)["y"].reshape(rows, C), y2.detach(), "apply y", 1e-10)
    _agree(fr["dx"].reshape(rows, C), x2.grad, "frozen dx", 1e-10)
    _agree(fr["dgamma"], g2.grad, "frozen dgamma", 1e-10)
    _agree(fr["dbeta"], b2.grad, "frozen dbeta", 1e-10)


@pytest.mark.parametrize("case", G.BN_CASES, ids=lambda c: c.name)
def test_batchnorm_two_formulations(case):
    p = G.bn_problem(case)
    _bn_two_formulations(p, p.act)


@pytest.mark.parametrize("act", R.ACTS)
def test_every_activation_two_formulations(act):
    """NONE, RELU, LEAKY, SILU, GELU on one small shape (the cases use four of them; GELU is part
    of the contract).  Kinked ones: the draw has no pre-activation at zero exactly, which is all
    the fp64 comparison needs."""
    _bn_two_formulations(G._bn_draw(G.BNCase(3, 100, 6, act, "scalar"), 1), act)


def _gn_two_formulations(p):
    N, HW, C, Gr = p.N, p.HW, p.C, p.groups
    x, g, b = (t.clone().requires_grad_() for t in (p.x, p.gamma, p.beta))
    y = _torch_act(p.act, F.group_norm(x.permute(0, 2, 1), Gr, g, b, p.eps).permute(0, 2, 1))
    y.backward(p.dy)
    f = p.fwd
    _agree(f["y"], y.detach(), "y")
    bw = R.chnorm_bwd(p.dy, p.x, f["mean"], f["rstd"], p.gamma, p.beta, Gr, 0, p.act)
    _agree(bw["dx"], x.grad, "dx")
    _agree(bw["dgamma"], g.grad, "dgamma")
    _agree(bw["dbeta"], b.grad, "dbeta")
    xg = R._per_group(p.x, Gr)
    _agree(f["mean"], xg.mean(1), "mean")
    _agree(f["rstd"], 1 / torch.sqrt(xg.var(1, unbiased=False) + p.eps), "rstd")


@pytest.mark.parametrize("case", G.GN_CASES, ids=lambda c: c.name)
def test_groupnorm_two_formulations(case):
    _gn_two_formulations(G.gn_problem(case))


# ---------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------
def _family(cases, problem, reference):
    for case in cases:
        p = problem(case)
        res = reference(p, torch.float32)
        for name, got in res.items():
            if name != "d":
                yield case, name, got, p


@pytest.fixture(scope="module")
def fp32_errors():
    """Per TOL entry: the largest normalised error of the fp32 restatement, and its case."""
    worst = {}
    families = ((G.LN_CASES + G.LN_EXACT_CASES, G.ln_problem, G.ln_reference), (G.BN_CASES, G.bn_problem, G.bn_reference),
                (G.GN_CASES, G.gn_problem, G.gn_reference))
    for cases, problem, reference in families:
        for case, name, got, p in _family(cases, problem, reference):
            e = G.normalised_error(got, p.ref[name], p.scale[name])
            key = G.tol_name(name)
            if e > worst.get(key, (-1.0, None))[0]:
                worst[key] = (e, case.name)
    return worst


def test_tolerances_come_from_the_fp32_restatement(fp32_errors):
    for name, (e, where) in sorted(fp32_errors.items()):
        print(f"{name:16s} fp32 restatement max {e:.3e} on {where}; TOL {G.TOL.get(name, float('nan')):.3e}")
    assert set(fp32_errors) == set(G.TOL) == set(G.MEASURED_FP32)
    for name, (e, where) in fp32_errors.items():
        tol, top = G.TOL[name], G.cap(name)
        assert tol <= top, name
        want = 4 * G.MEASURED_FP32[name]
        assert tol == top if want > top else want <= tol <= 1.1 * want, name
        if 2 * e > top:      # the cap binds whatever this machine's figure is
            assert tol == top, name
        else:
            assert 2 * e <= tol <= 8 * e, f"{name}: TOL {tol:.3e} is not 4 x {e:.3e} within a factor 2"


# ---------------------------------------------------------------------------------------------
# what the cases are named for
# ---------------------------------------------------------------------------------------------
def test_layernorm_cases_cover_every_instantiation():
    assert {G.ln_cache(c.C) for c in G.LN_CLASS_CASES} == {1, 2, 4, 8, 24}
    partly = {G.ln_cache(c.C) for c in G.LN_CLASS_CASES if (c.C // 4) % 64 != 0}
    full = {G.ln_cache(c.C) for c in G.LN_CLASS_CASES if (c.C // 4) % 64 == 0}
    assert partly == {1, 2, 4, 8, 24} and full >= {1, 24}
    assert all(c.rows % 4 != 0 for c in G.LN_CLASS_CASES)            # idle waves in the last block
    fwd_only, a, b = G.LN_STRIDE_CASES
    assert fwd_only.rows > G.ln_fwd_waves(fwd_only.rows) and not fwd_only.backward
    for c in (a, b):   # waves with two rows next to waves with one
        assert G.ln_bwd_waves(c.rows, c.C) < c.rows < 2 * G.ln_bwd_waves(c.rows, c.C)
    assert G.ln_bwd_waves(b.rows, b.C) == 4 * 512 and G.ln_cache(b.C) == 4
    assert G.ln_cache(6148) == -1 and G.ln_cache(6144) == 24


def _bn(N, HW, C):
    return next(c for c in G.BN_CASES if (c.N, c.HW, c.C) == (N, HW, C))


def test_batchnorm_case_geometry():
    stat = {c: G.bn_grid(c.rows, c.C, G.BN_STAT_BLOCKS) for c in G.BN_CASES if c.path == "vector"}
    appl = {c: G.bn_grid(c.rows, c.C, G.BN_APPLY_BLOCKS) for c in G.BN_CASES if c.path == "vector"}
    U, UA = G.BN_STATS_U, G.BN_APPLY_U

    c = _bn(2, 500, 24)
    assert stat[c].sq == 6 and G.BN_THREADS // 6 == 42 and G.BN_THREADS - 42 * 6 == 4 and stat[c].nsl == 1

    c = _bn(1, 2000, 256)    # a full chunk gives every thread U rows and no tail; the last chunk is short
    g = stat[c]
    assert g.sq == 64 and g.rpc == U * (G.BN_THREADS // 64)
    lengths = [G.bn_chunk_rows(g, k)[1] - G.bn_chunk_rows(g, k)[0] for k in range(g.nchunk)]
    assert set(lengths[:-1]) == {g.rpc} and 0 < lengths[-1] < g.rpc
    assert {n for _, n in G.bn_thread_rows(g)} == {U, lengths[-1] // 4}

    c = _bn(2, 4000, 1056)   # uneven last slice; U = 8 body + tail in the statistics; two U = 4 bodies in the apply
    assert G.bn_slices(stat[c]) == [53, 53, 53, 53, 52]
    assert {n for _, n in G.bn_thread_rows(stat[c]) if n} == {10} and U < 10 < 2 * U
    assert {n for _, n in G.bn_thread_rows(appl[c]) if n} == {2 * UA}

    c = _bn(4, 35, 520)      # uneven last slice; in the apply a U = 4 body and then a tail
    assert G.bn_slices(stat[c]) == [44, 44, 42] == G.bn_slices(appl[c])
    assert any(UA < n < 2 * UA for _, n in G.bn_thread_rows(appl[c]))
    assert c.act in R.KINKED

    c = _bn(1, 33000, 8)     # bn_reduce4: thread 0 sums >= U chunks, so its unrolled loop runs
    assert _cdiv(stat[c].nchunk, G.BN_THREADS) >= G.BN_REDUCE_U and stat[c].nchunk > 900

    c = _bn(1, 1, 8)
    assert c.rows == 1 and stat[c].nchunk == 1
    p = G.bn_problem(c)
    assert torch.equal(p.fwd["var"], torch.zeros(8, dtype=D))
    assert torch.equal(p.ref["bn.running_var"], (1 - p.momentum) * p.running_var0)

    # sq differs from g.sq only in an uneven last slice: both uneven cases have one
    assert sum(len(set(G.bn_slices(g))) > 1 for g in stat.values()) == 2
    for c in G.BN_CASES:
        if c.pooled:
            assert c.path == "vector" and c.C % 4 == 0
            gi = G.bn_grid_img(c.N, c.HW, c.C, G.BN_APPLY_BLOCKS)
            for k in range(gi.nchunk):   # no chunk straddles two images
                r0, r1 = G.bn_chunk_rows(gi, k)
                assert r0 < r1 and r0 // c.HW == (r1 - 1) // c.HW
    assert {(c.N, c.HW) for c in G.BN_POOLED_CASES} == {(3, 1), (3, 33)}
    for c in G.BN_SCALAR_CASES:
        assert c.C % 4 != 0
    assert any(c.C > G.BN_THREADS for c in G.BN_SCALAR_CASES)        # the c += CN_THREADS loop
    assert G.BN_MISALIGNED.C % 4 == 0 and G.MISALIGNED * 4 % 16 == 4
    assert G.ALIGNED * 4 % 16 == 0 and G.OFF16 * 4 % 16 == 8


def _cdiv(a, b):
    return -(-a // b)


def test_groupnorm_cases():
    small = [c for c in G.GN_CASES if c.HW * (c.C // c.groups) < G.BN_THREADS]
    assert {c.HW * (c.C // c.groups) for c in small} >= {2, 8, 72, 15}
    assert any(c.HW * (c.C // c.groups) > G.BN_THREADS for c in G.GN_CASES)
    assert any(c.groups == c.C for c in G.GN_CASES) and any(c.groups == 1 for c in G.GN_CASES)


def test_kinked_cases_exclude_nothing():
    kinked = [(c, G.bn_problem) for c in G.BN_CASES if c.act in R.KINKED]
    kinked += [(c, G.gn_problem) for c in G.GN_CASES if c.act in R.KINKED]
    assert len(kinked) == 4
    for case, problem in kinked:
        p = problem(case)
        print(f"{case.name}: seed {p.seed}, margin {p.margin:.3e}, elements within it {p.near}")
        assert p.near == 0 and p.margin > 0
    big = [c for c in G.BN_CASES + G.GN_CASES if c.N * c.HW * c.C > 100000]
    assert big and all(c.act in (R.ACT_NONE, R.ACT_SILU) for c in big)


# ---------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------
def _ln(rows, C):
    return G.ln_problem(next(c for c in G.LN_CASES if (c.rows, c.C) == (rows, C)))


def _rejected(p, bad, names=None):
    return [n for n in (names or bad) if n != "d" and not G.passes(n, bad[n], p.ref[n], p.scale[n])]


def _f32(res):
    return {n: t.float() for n, t in res.items()}


def _clean_passes(p, reference, dtype=torch.float32):
    assert _rejected(p, _f32(reference(p, dtype))) == [], "the restatement itself fails"


@pytest.mark.parametrize("flaw,where,name", [("var_c_minus_1", (5, 4), "ln.y"), ("eps_outside_sqrt", (5, 384), "ln.rstd"),
                                             ("dx_without_m2", (5, 768), "ln.dx")])
def test_layernorm_formula_flaws_fail(flaw, where, name):
    p = _ln(*where)
    _clean_passes(p, G.ln_reference)
    rejected = _rejected(p, G.ln_reference(p, torch.float32, (flaw,)))
    print(f"{flaw}: rejected by {rejected}")
    assert name in rejected


def test_layernorm_dgamma_missing_second_visit_fails():
    p = _ln(4101, 64)
    waves = G.ln_bwd_waves(p.rows, p.C)
    first = R.layernorm_bwd(p.dy[:waves], p.x[:waves], p.mean32[:waves], p.rstd32[:waves], p.gamma, torch.float32)
    assert not G.passes("ln.dgamma", first["dgamma"], p.ref["ln.dgamma"], p.scale["ln.dgamma"])
    assert not G.passes("ln.dbeta", first["dbeta"], p.ref["ln.dbeta"], p.scale["ln.dbeta"])


def test_layernorm_arm_flaws_fail():
    p = G.ln_problem(G.LN_ARMS)
    res = G.ln_reference(p, torch.float32)
    assert not G.passes("ln.dgamma", res["ln.dbeta"], p.ref["ln.dgamma"], p.scale["ln.dgamma"])      # swapped
    assert not G.passes("ln.dbeta", res["ln.dgamma"], p.ref["ln.dbeta"], p.scale["ln.dbeta"])
    dx = res["ln.dx"].double()
    for add in (p.dx0, p.dadd):
        want, scale = p.ref["ln.dx"] + add, G.ln_dx_scale(p, add)
        assert G.passes("ln.dx", (dx + add).float(), want, scale)
        assert not G.passes("ln.dx", dx.float(), want, scale)                  # accumulate_dx ignored
        assert not G.passes("ln.dx", (dx + 2 * add).float(), want, scale)      # dadd added twice when aliased


@pytest.mark.parametrize("flaw,where,name", [("running_var_biased", (3, 100, 6), "bn.running_var"),
                                             ("momentum_reversed", (2, 500, 24), "bn.running_mean"),
                                             ("inv_n_rows_minus_1", (3, 100, 6), "bn.dx"),
                                             ("silu_grad_at_y", (2, 500, 24), "bn.dx")])
def test_batchnorm_formula_flaws_fail(flaw, where, name):
    p = G.bn_problem(_bn(*where))
    # in fp64, rounded to fp32: the sequential fp32 sums themselves miss the capped forward
    # tolerances on channels shifted by 100 spreads
    _clean_passes(p, G.bn_reference, D)
    rejected = _rejected(p, _f32(G.bn_reference(p, D, (flaw,))))
    print(f"{flaw}: rejected by {rejected}")
    assert name in rejected
    if flaw == "running_var_biased":
        assert "bn.ru_running_var" in rejected
    if flaw == "silu_grad_at_y":
        assert {"bn.dgamma", "bn.dbeta", "bn.frozen_dx"} <= set(rejected)


def test_batchnorm_partition_flaws_fail():
    case = _bn(2, 500, 24)
    p = G.bn_problem(case)
    res = _f32(G.bn_reference(p, D))
    # one chunk's partial dropped from dbeta
    g = G.bn_grid(p.rows, p.C, G.BN_STAT_BLOCKS)
    assert g.nchunk > 4
    r0, r1 = G.bn_chunk_rows(g, 3)
    dropped = res["bn.dbeta"].double() - res["d"].double().reshape(p.rows, p.C)[r0:r1].sum(0)
    assert not G.passes("bn.dbeta", dropped.float(), p.ref["bn.dbeta"], p.scale["bn.dbeta"])
    # pooled divided by the chunk length instead of HW
    gi = G.bn_grid_img(p.N, p.HW, p.C, G.BN_APPLY_BLOCKS)
    assert gi.rpc != p.HW
    assert G.passes("bn.pooled", res["bn.pooled"], p.ref["bn.pooled"], p.scale["bn.pooled"])
    assert not G.passes("bn.pooled", res["bn.pooled"] * (p.HW / gi.rpc), p.ref["bn.pooled"], p.scale["bn.pooled"])
    # the last slice's channels normalised with the previous slice's statistics
    p = G.bn_problem(_bn(4, 35, 520))
    g = G.bn_grid(p.rows, p.C, G.BN_APPLY_BLOCKS)
    last = 4 * g.sq * (g.nsl - 1)
    mean, rstd = p.fwd["mean"].clone(), p.fwd["rstd"].clone()
    mean[last:], rstd[last:] = mean[last - 4 * g.sq:p.C - 4 * g.sq], rstd[last - 4 * g.sq:p.C - 4 * g.sq]
    y = R.chnorm_apply(p.x, p.gamma, p.beta, mean, rstd, p.C, 1, p.act, torch.float32)["y"]
    assert not G.passes("bn.y", y, p.ref["bn.y"], p.scale["bn.y"])
    good = R.chnorm_apply(p.x, p.gamma, p.beta, p.fwd["mean"], p.fwd["rstd"], p.C, 1, p.act, torch.float32)["y"]
    assert G.passes("bn.y", good, p.ref["bn.y"], p.scale["bn.y"])


@pytest.mark.parametrize("flaw", R.FLAWS_GN)
def test_groupnorm_flaws_fail(flaw):
    p = G.gn_problem(next(c for c in G.GN_CASES if (c.HW, c.C, c.groups) == (300, 64, 4)))
    _clean_passes(p, G.gn_reference)
    rejected = _rejected(p, G.gn_reference(p, torch.float32, (flaw,)))
    print(f"{flaw}: rejected by {rejected}")
    # the backward takes its statistics as inputs: only the group index reaches it
    assert ({"gn.y", "gn.mean", "gn.rstd"} if flaw == "stats_whole_sample" else {"gn.y", "gn.apply_y", "gn.dx"}) <= set(rejected)


def test_truncated_bf16_copy_fails_bit_equality():
    p = _ln(5, 384)
    y = p.ref["ln.y"].float()
    assert torch.equal(R.bf16_rne(y), y.to(torch.bfloat16))
    trunc = R.bf16_truncated(y)
    assert not torch.equal(trunc, y.to(torch.bfloat16))
    # truncation is a legitimate bf16 neighbour of every element: only the bit-equality rule sees it
    assert ((trunc.float() - y).abs() <= y.abs() * 2.0 ** -7).all().item()


def test_exact_layernorm_cases_are_exact_in_the_reference():
    for case in G.LN_EXACT_CASES:
        p = G.ln_problem(case)
        if case.kind == "const":
            assert torch.equal(p.ref["ln.y"], p.beta[None, :].expand(p.rows, p.C))
            assert torch.equal(p.ref["ln.mean"], torch.tensor(G.CONST_VALUES, dtype=D))
        else:
            assert case.C & (case.C - 1) == 0
            assert torch.equal(p.ref["ln.mean"], torch.zeros(p.rows, dtype=D))
            assert torch.equal(p.ref["ln.y"], p.x * p.ref["ln.rstd"][:, None])
