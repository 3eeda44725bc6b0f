"""Reference of the normalisation entry points of include/mdemi.h (LayerNorm, BatchNorm,
GroupNorm, the running-statistics update, the pooled BatchNorm apply), restated from the header
text -- not from the kernels -- in plain torch on the CPU.

dtype=torch.float64 is the reference the GPU tests compare with.  dtype=torch.float32 runs the
same formulas in fp32 with every reduction over rows, channels or pixels taken as a sequential
fp32 sum (seqsum: one rounded addition per term, in index order).  That is the least accurate
order any kernel of the family uses -- they sum per lane and then by a tree, or in fp64 -- so the
error of this restatement against the fp64 one bounds theirs; the tolerances of
tests/norm_contract_cases.py are 4 x that error.  (torch.cumsum on a CPU float tensor keeps its
running sum in double, so it is not such a sum; seqsum loops.)

Conventions: LayerNorm works on x [rows, C]; the channel norms on x [N, HW, C] (NHWC).  Statistics
handed to a backward are inputs of that call: the reference uses the values it is given (the
fp32 numbers the kernel reads), not statistics of its own.

`flaws` plants one wrong result per name (FLAWS_*): test_norm_contract_ref.py shows that the
criterion of norm_contract_cases rejects each of them."""
import math

import torch

ACT_NONE, ACT_GELU, ACT_RELU, ACT_LEAKY, ACT_SILU = 0, 1, 2, 3, 6
ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SILU, ACT_GELU)
KINKED = (ACT_RELU, ACT_LEAKY)
LEAKY_SLOPE = 0.01

FLAWS_LN = ("var_c_minus_1", "eps_outside_sqrt", "dx_without_m2")
FLAWS_BN = ("running_var_biased", "momentum_reversed", "inv_n_rows_minus_1", "silu_grad_at_y")
FLAWS_GN = ("stats_whole_sample", "group_index_mod")


def seqsum(t, dim):
    """Sum over `dim`: fp64 -> torch.sum; fp32 -> one rounded addition per term, in order."""
    if t.dtype == torch.float64:
        return t.sum(dim)
    t = t.movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def seqmean(t, dim):
    return seqsum(t, dim) / t.shape[dim]


def act_fwd(act, v):
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, LEAKY_SLOPE * v)
    if act == ACT_SILU:
        return v / (1 + torch.exp(-v))
    if act == ACT_GELU:
        return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    assert act == ACT_NONE
    return v


def act_grad(act, v):
    """d act / d v at the pre-activation v."""
    if act == ACT_RELU:
        return (v > 0).to(v.dtype)
    if act == ACT_LEAKY:
        return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, LEAKY_SLOPE))
    if act == ACT_SILU:
        s = 1 / (1 + torch.exp(-v))
        return s + v * s * (1 - s)
    if act == ACT_GELU:
        return 0.5 * (1 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    assert act == ACT_NONE
    return torch.ones_like(v)


# ---------------------------------------------------------------------------------------------
# LayerNorm over the last dimension
# ---------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, dtype=torch.float64, flaws=()):
    """y = (x - mean) * rstd * gamma + beta, mean / rstd [rows] from the biased variance."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    C = x.shape[1]
    mean = seqsum(x, 1) / C
    xc = x - mean[:, None]
    var = seqsum(xc * xc, 1) / ((C - 1) if "var_c_minus_1" in flaws else C)
    rstd = 1 / (torch.sqrt(var) + eps) if "eps_outside_sqrt" in flaws else 1 / torch.sqrt(var + eps)
    xhat = xc * rstd[:, None]
    return dict(y=xhat * gamma + beta, mean=mean, rstd=rstd, xhat=xhat)


def layernorm_bwd(dy, x, mean, rstd, gamma, dtype=torch.float64, flaws=(), add=None):
    """dx = rstd * (g dy - mean_c(g dy) - xhat * mean_c(g dy xhat)) (+ add: the old dx of
    accumulate_dx = 1, or dadd of mdemi_layernorm_bwd_add); dgamma = sum_rows dy xhat,
    dbeta = sum_rows dy."""
    dy, x, mean, rstd, gamma = (t.to(dtype) for t in (dy, x, mean, rstd, gamma))
    xhat = (x - mean[:, None]) * rstd[:, None]
    gd = dy * gamma
    m1 = seqmean(gd, 1)[:, None]
    m2 = seqmean(gd * xhat, 1)[:, None]
    dx = rstd[:, None] * (gd - m1 - (0 if "dx_without_m2" in flaws else xhat * m2))
    if add is not None:
        dx = dx + add.to(dtype)
    return dict(dx=dx, dgamma=seqsum(dy * xhat, 0), dbeta=seqsum(dy, 0), xhat=xhat)


# ---------------------------------------------------------------------------------------------
# Channel normalisation over NHWC: BatchNorm (statistics per channel over N, HW) and GroupNorm
# (per (n, group) over HW and the group's C / groups channels)
# ---------------------------------------------------------------------------------------------
def _per_group(t, groups):
    """[N, HW, C] -> [N * groups, HW * cpg] (the elements one GroupNorm statistic covers)."""
    N, HW, C = t.shape
    return t.reshape(N, HW, groups, C // groups).permute(0, 2, 1, 3).reshape(N * groups, -1)


def stat_index(N, C, groups, is_bn, flaws=()):
    """[N, C] index of the statistic that normalises channel c of sample n."""
    c = torch.arange(C)
    if is_bn:
        return c[None, :].expand(N, C)
    g = c % groups if "group_index_mod" in flaws else c // (C // groups)
    return torch.arange(N)[:, None] * groups + g[None, :]


def expand_stat(stat, N, C, groups, is_bn, flaws=()):
    """mean / rstd ([C] or [N * groups]) broadcast to [N, 1, C]."""
    return stat[stat_index(N, C, groups, is_bn, flaws)][:, None, :]


def chnorm_stats(x, groups, is_bn, eps, dtype=torch.float64, flaws=()):
    x = x.to(dtype)
    N, HW, C = x.shape
    if is_bn:
        flat = x.reshape(N * HW, C)
        mean = seqsum(flat, 0) / flat.shape[0]
        xc = flat - mean
        var = seqsum(xc * xc, 0) / flat.shape[0]
    else:
        flat = _per_group(x, 1 if "stats_whole_sample" in flaws else groups)
        mean = seqsum(flat, 1) / flat.shape[1]
        xc = flat - mean[:, None]
        var = seqsum(xc * xc, 1) / flat.shape[1]
        if "stats_whole_sample" in flaws:
            mean, var = mean.repeat_interleave(groups), var.repeat_interleave(groups)
    return mean, 1 / torch.sqrt(var + eps), var


def chnorm_apply(x, gamma, beta, mean, rstd, groups, is_bn, act, dtype=torch.float64, flaws=()):
    """mdemi_chnorm_apply: y = act((x - mean) * rstd * gamma + beta) with the given statistics."""
    x, gamma, beta, mean, rstd = (t.to(dtype) for t in (x, gamma, beta, mean, rstd))
    N, HW, C = x.shape
    xhat = (x - expand_stat(mean, N, C, groups, is_bn, flaws)) * expand_stat(rstd, N, C, groups, is_bn, flaws)
    pre = xhat * gamma + beta
    return dict(y=act_fwd(act, pre), pre=pre, xhat=xhat)


def chnorm_fwd(x, gamma, beta, groups, is_bn, eps, act, dtype=torch.float64, flaws=()):
    mean, rstd, var = chnorm_stats(x, groups, is_bn, eps, dtype, flaws)
    out = chnorm_apply(x, gamma, beta, mean, rstd, groups, is_bn, act, dtype, flaws)
    out.update(mean=mean, rstd=rstd, var=var)
    return out


def running_update(mean, var, running_mean, running_var, rows, momentum, dtype=torch.float64, flaws=()):
    """nn.BatchNorm2d in training: running = (1 - m) running + m batch, the batch variance
    unbiased (rows / (rows - 1); 1 for a single row)."""
    mean, var, rm, rv = (t.to(dtype) for t in (mean, var, running_mean, running_var))
    unbias = 1.0 if rows == 1 or "running_var_biased" in flaws else rows / (rows - 1)
    keep, take = (momentum, 1 - momentum) if "momentum_reversed" in flaws else (1 - momentum, momentum)
    return dict(running_mean=keep * rm + take * mean, running_var=keep * rv + take * var * unbias)


def bn_running_update(mean, rstd, running_mean, running_var, rows, eps, momentum, dtype=torch.float64, flaws=()):
    """mdemi_bn_running_update: the same from the batch mean / rstd (var = 1 / rstd^2 - eps)."""
    rstd = rstd.to(dtype)
    return running_update(mean, 1 / (rstd * rstd) - eps, running_mean, running_var, rows, momentum, dtype, flaws)


def bn_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, act, dtype=torch.float64, flaws=()):
    """mdemi_bn_train_fwd / _fwd16 / _fwd_pooled: chnorm_fwd (BatchNorm), the running update,
    pooled [N, C] = the mean of y over HW."""
    N, HW, C = x.shape
    out = chnorm_fwd(x, gamma, beta, C, 1, eps, act, dtype, flaws)
    out.update(running_update(out["mean"], out["var"], running_mean, running_var, N * HW, momentum, dtype, flaws))
    out["pooled"] = seqsum(out["y"], 1) / HW
    return out


def chnorm_bwd(dy, x, mean, rstd, gamma, beta, groups, is_bn, act, dtype=torch.float64, flaws=()):
    """d = dy * act'(pre), pre = xhat gamma + beta from the given statistics;
    dgamma = sum d xhat, dbeta = sum d over N, HW;
    BatchNorm: dx = gamma rstd (d - dbeta / n - xhat dgamma / n), n = N * HW;
    GroupNorm: dx = rstd (g d - mean_grp(g d) - xhat mean_grp(g d xhat))."""
    dy = dy.to(dtype)
    N, HW, C = dy.shape
    f = chnorm_apply(x, gamma, beta, mean, rstd, groups, is_bn, act, dtype, flaws)
    xhat, gamma = f["xhat"], gamma.to(dtype)
    at = f["y"] if (act == ACT_SILU and "silu_grad_at_y" in flaws) else f["pre"]
    d = dy * act_grad(act, at)
    dgamma = seqsum((d * xhat).reshape(N * HW, C), 0)
    dbeta = seqsum(d.reshape(N * HW, C), 0)
    rs = expand_stat(rstd.to(dtype), N, C, groups, is_bn, flaws)
    if is_bn:
        inv_n = 1.0 / ((N * HW - 1) if "inv_n_rows_minus_1" in flaws else N * HW)
        dx = gamma * rs * (d - inv_n * dbeta - xhat * (inv_n * dgamma))
    else:
        gd = d * gamma
        cnt = HW * (C // groups)
        m1 = seqsum(_per_group(gd, groups), 1) / cnt
        m2 = seqsum(_per_group(gd * xhat, groups), 1) / cnt
        dx = rs * (gd - expand_stat(m1, N, C, groups, 0) - xhat * expand_stat(m2, N, C, groups, 0))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, d=d, xhat=xhat, pre=f["pre"])


def bn_frozen_bwd(dy, x, mean, rstd, gamma, beta, act, dtype=torch.float64, flaws=()):
    """mdemi_bn_frozen_bwd: dx = gamma rstd act'(pre) dy; dgamma / dbeta as in training."""
    N, HW, C = dy.shape
    b = chnorm_bwd(dy, x, mean, rstd, gamma, beta, C, 1, act, dtype, flaws)
    b["dx"] = gamma.to(dtype) * rstd.to(dtype) * b["d"]
    return b


# ---------------------------------------------------------------------------------------------
# bf16 copies
# ---------------------------------------------------------------------------------------------
def bf16_rne(t32):
    """The copy the header promises: round to nearest even."""
    return t32.to(torch.bfloat16)


def bf16_truncated(t32):
    """A copy made by dropping the low 16 bits (the planted error of the bit-equality rule)."""
    bits = t32.contiguous().view(torch.int32) >> 16
    return bits.to(torch.int16).view(torch.bfloat16)
